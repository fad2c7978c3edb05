// Workspace layouts of the C-ABI (internal): every caller-provided workspace is carved by ONE function, which the size
// query runs on a null base and the entry point on the caller's pointer.  (A layout that lies behind the Work of the same
// call is carved by one function too: it starts its Carve at the Work's size.)
#pragma once
#include <algorithm>
#include <type_traits>
#include <vector>

#include "sf_band_shape.h"
#include "sf_ctx.h"

struct Carve {
    char* base;
    size_t off, cap;
    Carve(void* p, size_t bytes, size_t start = 0) : base((char*)p), off(start), cap(bytes) {}
    template <typename T>
    T* take(size_t count) {
        off = sf_align_up(off, 256);
        T* r = base ? (T*)(base + off) : nullptr;
        off += sizeof(T) * count;
        return r;
    }
};
static int work_fits(size_t have, size_t need) {
    if (have < need) {
        sf_set_error("workspace too small: have %zu, need %zu", have, need);
        return SF_ENOMEM;
    }
    return SF_OK;
}
// Row strides / per-unit sizes of the batched buffers.  A single-order call uses the order's own padding; a
// multi-order call (sf_loglike_multi_batch) pads every order to the largest one of the group so that all
// units share ONE batched factorisation.
struct Layout {
    int m, mpad, M, nf, rows, npad, lda;
};
static size_t tilemap_bytes(const Layout& L) {  // per unit: one byte per 128 x 128 tile, as the kernels index it
    const size_t nt128 = (size_t)(L.npad + 127) / 128;  // (the same count in the frame shifted by 64: npad = 64 mod 128 there)
    return nt128 * nt128;
}
static Layout layout_of(const sf_ctx* c) { return Layout{c->m, c->mpad, c->M, c->nf, c->rows, c->npad, c->lda}; }
struct Work {
    double *mu, *Lw, *zs, *kv, *scale, *logdet, *sqmah, *coef, *ybro, *Xraw, *fraw, *resid, *Y, *C, *ltbuf, *mult, *gtab;
    double2* fft;
    int *info_e, *info_c;
    unsigned char* tilemap;
    unsigned* tilelist;        // compact list of the materialised tiles (see sf_fill_args)
    int* tilecount;
    unsigned char* dmap;       // dense fill of caller matrices: structured-support map / list of 64 x 64 tiles
    unsigned short* dlist;
    int* dcount;
    size_t bytes;
    Layout L;
    int trans_bt = 0;      // walkers one set of transient buffers is sized for
    size_t fft_set = 0;    // double2 per set
};
// The buffers of Work in carve order: f(pointer, elements, present, kind).
//   PER_UNIT  `elements` per unit; a slice of the units [u0, ...) starts u0 * elements further on
//   PER_SET   `elements` per set of the transient buffers of the transform chain (used by one launch sequence at a time,
//             stream ordered; one set per lane of a multi-order call)
//   SHARED    one per workspace, sized by carve
enum WorkKind { PER_UNIT, PER_SET, SHARED };
template <class F>
static void work_buffers(Work& w, bool has_vsini, bool need_C, F&& f) {
    const Layout& L = w.L;
    const size_t npad = (size_t)L.npad, bt = (size_t)w.trans_bt;
    f(w.mu, (size_t)L.m, true, PER_UNIT);
    f(w.Lw, (size_t)L.m * L.m, true, PER_UNIT);
    f(w.zs, (size_t)L.m * L.M * L.m, true, PER_UNIT);
    f(w.kv, (size_t)L.m * L.M, true, PER_UNIT);
    f(w.scale, 1, true, PER_UNIT);
    f(w.logdet, 1, true, PER_UNIT);
    f(w.sqmah, 1, true, PER_UNIT);
    f(w.info_e, 1, true, PER_UNIT);
    f(w.info_c, 1, true, PER_UNIT);
    f(w.coef, bt * L.nf * L.rows, has_vsini, PER_SET);
    f(w.ybro, bt * L.nf * L.rows, has_vsini, PER_SET);  // broadened rows before the fit
    f(w.mult, bt * (L.nf / 2 + 1), has_vsini, PER_SET);  // broadening kernel per walker
    f(w.fft, w.fft_set, w.fft_set != 0, PER_SET);
    f(w.Xraw, L.m * npad, true, PER_UNIT);
    f(w.fraw, npad, true, PER_UNIT);
    f(w.resid, npad, true, PER_UNIT);
    f(w.Y, L.mpad * npad, true, PER_UNIT);
    double* reserved = nullptr;  // npad doubles per unit that nothing reads (once the z of a separate triangular solve):
    f(reserved, npad, true, PER_UNIT);  // kept so that C and the Cholesky scratch stay at the offsets they were measured at
    f(w.ltbuf, 0, need_C, SHARED);  // Cholesky scratch
    f(w.tilemap, tilemap_bytes(L), need_C, PER_UNIT);
    f(w.tilelist, tilemap_bytes(L), need_C, PER_UNIT);  // (capacity: every tile)
    f(w.tilecount, 1, need_C, PER_UNIT);
    f(w.gtab, npad, need_C, PER_UNIT);
    f(w.dmap, sf_fill_dense_map_tiles(L.npad), true, PER_UNIT);
    f(w.dlist, sf_fill_dense_map_tiles(L.npad), true, PER_UNIT);
    f(w.dcount, 1, true, PER_UNIT);
    f(w.C, npad * L.lda, need_C, PER_UNIT);
}
// B units of per-unit buffers; the transient buffers are sized for Bt walkers, trans_sets independent sets of them (for
// transform chains running side by side); the Cholesky scratch for potrf_units matrices per factorisation (0: all B)
static Work carve(const Layout& L, const sf_model_desc* mdl, int B, int Bt, void* p, size_t cap, bool need_C,
                  int potrf_units = 0, int trans_sets = 1) {
    Carve k(p, cap);
    Work w{};
    w.L = L;
    w.trans_bt = Bt;
    w.fft_set = (mdl->has_vsini ? sf_fft_half_scratch_bytes(Bt * L.rows, L.nf) : 0) / sizeof(double2);
    const size_t ltbuf = sf_align_up(sf_potrf_work_doubles(L.npad, potrf_units > 0 ? potrf_units : B), 32);
    work_buffers(w, mdl->has_vsini != 0, need_C, [&](auto*& ptr, size_t elements, bool present, WorkKind kind) {
        using T = std::remove_reference_t<decltype(*ptr)>;
        const size_t count = kind == PER_UNIT ? (size_t)B * elements : kind == PER_SET ? (size_t)trans_sets * elements : ltbuf;
        ptr = present ? k.take<T>(count) : nullptr;
    });
    w.bytes = sf_align_up(k.off, 256);
    return w;
}
static Work carve(const sf_ctx* c, const sf_model_desc* mdl, int B, void* p, size_t cap, bool need_C) {
    return carve(layout_of(c), mdl, B, B, p, cap, need_C);
}
// the buffers of the units [u0, ...) of a multi-order workspace (transient buffers are shared)
static Work slice(const Work& w, int u0) {
    Work s = w;
    work_buffers(s, false, false, [&](auto*& ptr, size_t elements, bool, WorkKind kind) {
        if (ptr && kind == PER_UNIT) ptr += (size_t)u0 * elements;
    });
    return s;
}
// set `set` of the transient buffers (multi-order calls run several orders' transform chains side by side)
static Work with_trans_set(const Work& w, int set) {
    Work s = w;
    work_buffers(s, false, false, [&](auto*& ptr, size_t elements, bool, WorkKind kind) {
        if (ptr && kind == PER_SET) ptr += (size_t)set * elements;
    });
    return s;
}

// ------------------------------------------------------------------- structure-exploiting solver
// (behind the Work of the same call: base_bytes = its size)
struct BandWork {
    double *band, *gram, *logdet_band, *twist, *gtab, *tiles;
    int ldb;
    size_t bytes;
};
static BandWork carve_band(const sf_ctx* c, int B, int halfwidth, void* p, size_t cap, size_t base_bytes) {
    Carve k(p, cap, base_bytes);
    BandWork w;
    // Half-widths beyond the LDS window are factorised as bordered band matrices on the tile kernels of the dense
    // path (sf_launch_potrf_band); the band fill writes those tiles directly.
    const bool tiles = sfb_admit(halfwidth, c->m + 1) != SFB_WINDOW;
    w.ldb = tiles ? 128 * (sf_band_tiles_wt(halfwidth) + 1) : ((halfwidth + 2) & ~1);
    w.band = tiles ? nullptr : k.take<double>((size_t)B * c->npad * w.ldb);  // (the tiles are filled directly)
    w.gram = k.take<double>((size_t)B * (c->m + 1) * (c->m + 1));
    w.logdet_band = k.take<double>((size_t)B);
    w.twist = tiles ? nullptr : k.take<double>(sfb_twist_carve(nullptr, halfwidth, c->m + 1, B).doubles);
    w.gtab = k.take<double>((size_t)B * (w.ldb + 2));
    w.tiles = tiles ? k.take<double>(sf_band_tiles_doubles(c->npad, B)) : nullptr;
    w.bytes = sf_align_up(k.off, 256);
    return w;
}

// ------------------------------------------------------------------- the factor applied to right-hand sides
// (sf_apply_batch, sf_decompose_batch, sf_pointwise_batch, sf_loglike_grad_batch, sf_fisher_cov_batch,
// sf_loglike_mean_grad_batch, sf_local_scan_batch; behind the Work of the same call: base_bytes = its size)  Every call has the staging area -- the right-hand sides padded to npad rows, the factor is applied
// to it in place (for all but sf_apply_batch it ends up holding alpha = C^-1 rhs) -- and lnl / info, what the likelihood's
// last step leaves.  Then, in this order, the parts the call asks for:
//   AW_YV        yv: t = Y alpha, m doubles per right-hand side (sf_decompose_batch)
//   AW_COV_DIAG  cov_diag: the diagonal of the matrix that is factorised, npad doubles per walker (sf_pointwise_batch)
//   AW_INVERSE   cinv_diag: the diagonal of the inverse, npad doubles per walker (the inverse's launch writes it; the
//                gradient does not read it), and winv: the scratch of that launch (carve_potri)
//   AW_PART      part: the gradient's partial sums per (walker, block row, slot)
//   AW_MEAN      (sf_loglike_mean_grad_batch, nslots slots) xs: the m scaled rows X of every walker, n doubles each; fin: its
//                moments (sf_mean_fin_doubles); mpart: the partial sums per (walker, 256-pixel block, slot); dcoef: the spline
//                coefficients of the d / d vsini rows (models with vsini); kdot, mudot, zdot: d v12, d mu and Linv d v12 for
//                min(nslots, P) grid columns
//   AW_FISHER    (sf_fisher_mean_batch, with AW_MEAN) fpart: the partial sums of Z^T Z per (walker, 256-pixel block, pair of slots)
//   AW_FISHER_COV  (sf_fisher_cov_batch, with AW_INVERSE and AW_PART) wfull: every tile of W = C^-1, both triangles, and tj: one
//                T_j = W dC_j, ld x ld doubles per walker each with ld = sf_fisher_cov_ld(n) <= npad -- the same for every number
//                of slots: the slots are worked through one at a time, and part holds the sums of the slot at hand
//   AW_LOCAL_SCAN  (sf_local_scan_batch, with AW_INVERSE; nslots = its candidates) patch: two ints per candidate, the first and
//                last pixel in its reach; wband: per walker and 64-row block A the 64 x 64 tiles (A, K) of W = C^-1 for |A - K| <=
//                reach = min(blocks - 1, 4), [B][blocks][2 reach + 1][64][64] doubles (sf_local_scan_band_doubles) -- linear in n
enum AppliedParts {
    AW_YV = 1, AW_COV_DIAG = 2, AW_INVERSE = 4, AW_PART = 8, AW_MEAN = 16, AW_FISHER = 32, AW_FISHER_COV = 64, AW_LOCAL_SCAN = 128
};
struct AppliedWork {
    double *stage, *lnl;
    int* info;
    double *yv, *cov_diag, *cinv_diag, *winv, *part, *xs, *fin, *mpart, *dcoef, *kdot, *mudot, *zdot, *fpart, *wfull, *tj;
    int* patch;    // (AW_LOCAL_SCAN)
    double* wband;
    double* coef;  // (carve_multi_grad only) the segment's own spline coefficients, which a single-order call keeps in its Work
    size_t bytes;
};
static AppliedWork carve_applied(const sf_ctx* c, const sf_model_desc* mdl, int B, int nrhs, unsigned parts, void* p, size_t cap,
                                 size_t base_bytes, int nslots = 0) {
    Carve k(p, cap, base_bytes);
    AppliedWork w{};
    w.stage = k.take<double>((size_t)B * nrhs * c->npad);
    w.lnl = k.take<double>((size_t)B);
    w.info = k.take<int>((size_t)B);
    if (parts & AW_YV) w.yv = k.take<double>((size_t)B * nrhs * c->m);
    if (parts & AW_COV_DIAG) w.cov_diag = k.take<double>((size_t)B * c->npad);
    if (parts & AW_INVERSE) {
        w.cinv_diag = k.take<double>((size_t)B * c->npad);
        w.winv = k.take<double>(sf_chol_inverse_work_doubles(c->npad, B));
    }
    if (parts & AW_PART) w.part = k.take<double>(sf_cov_grad_work_doubles(c->n, mdl->has_global, mdl->n_local, B));
    if (parts & AW_MEAN) {
        w.xs = k.take<double>((size_t)B * c->m * c->n);
        w.fin = k.take<double>((size_t)B * sf_mean_fin_doubles(c->m));
        w.mpart = k.take<double>(sf_mean_grad_part_doubles(c->n, nslots, B));
        if (mdl->has_vsini) w.dcoef = k.take<double>((size_t)B * c->nf * c->rows);
        const size_t ng = (size_t)(nslots < c->P ? nslots : c->P), mM = (size_t)c->m * c->M;
        w.kdot = k.take<double>(ng * B * mM);
        w.mudot = k.take<double>(ng * B * c->m);
        w.zdot = k.take<double>(ng * B * mM * c->m);
    }
    if (parts & AW_FISHER) w.fpart = k.take<double>(sf_fisher_part_doubles(c->n, nslots, B));
    if (parts & AW_FISHER_COV) {
        const size_t ld = (size_t)sf_fisher_cov_ld(c->n);
        w.wfull = k.take<double>((size_t)B * ld * ld);
        w.tj = k.take<double>((size_t)B * ld * ld);
    }
    if (parts & AW_LOCAL_SCAN) {
        w.patch = k.take<int>(2 * (size_t)nslots);
        w.wband = k.take<double>(sf_local_scan_band_doubles(c->n, B));
    }
    w.bytes = sf_align_up(k.off, 256);
    return w;
}

// ------------------------------------------------------------------- the full banded solve
// sf_band_solve_batch: what the keeping sweep stores (sfb_keep_doubles per matrix), then the Gram matrices of a call that
// asks for none
struct BandSolveWork {
    double *fac, *gram;
    size_t bytes;
};
static BandSolveWork carve_band_solve(int n, int halfwidth, int batch, int nrhs, void* p, size_t cap) {
    Carve k(p, cap);
    BandSolveWork w;
    w.fac = k.take<double>((size_t)batch * sfb_keep_doubles(n, sfb_nbr(halfwidth), sfb_nrb(nrhs)));
    w.gram = k.take<double>((size_t)batch * nrhs * nrhs);
    w.bytes = sf_align_up(k.off, 256);
    return w;
}
// sf_band_selinv_batch: the keeping sweep's records for one right-hand side, that right-hand side (n zeros, shared by the batch)
// and its Gram matrices (one double per matrix)
struct BandSelinvWork {
    double *fac, *gram, *zero;
    size_t bytes;
};
static BandSelinvWork carve_band_selinv(int n, int halfwidth, int batch, void* p, size_t cap) {
    Carve k(p, cap);
    BandSelinvWork w;
    w.fac = k.take<double>((size_t)batch * sfb_keep_doubles(n, sfb_nbr(halfwidth), 1));
    w.gram = k.take<double>((size_t)batch);
    w.zero = k.take<double>((size_t)n);
    w.bytes = sf_align_up(k.off, 256);
    return w;
}
// sf_loglike_banded_mean_grad_batch and sf_loglike_banded_grad_batch, behind the Work of the same call: the band solver's
// buffers (carve_band), the mean gradient's (carve_applied with AW_MEAN: the staging area [alpha, V], lnl, info, xs, fin, ...),
// then fac: the kept factor of the sweep over n16 = n rounded up to whole blocks; T: [B][1 + m][npad] = Bd^-1 [r, Y^T]; M:
// [B][(1 + m)^2] mix matrices.  Behind them, for a call that wants the covariance slots (NULL otherwise), sigma: the band of
// Bd^-1, [B][n16][bw.ldb]; M2, stage2: the mix matrix of Vs and [0, Vs] in the staging layout [B][1 + m][npad]; part: the
// contraction's partial sums (sf_cov_grad_work_doubles)
struct BandGradWork {
    BandWork bw;
    AppliedWork aw;
    double *fac, *T, *M;
    double *sigma, *M2, *stage2, *part;
    size_t bytes;
};
static BandGradWork carve_band_grad(const sf_ctx* c, const sf_model_desc* mdl, int B, int halfwidth, int nslots, bool want_cov, void* p,
                                    size_t cap, size_t base_bytes) {
    BandGradWork g{};
    const int nrhs = c->m + 1, n16 = (c->n + 15) / 16 * 16;
    g.bw = carve_band(c, B, halfwidth, p, cap, base_bytes);
    g.aw = carve_applied(c, mdl, B, nrhs, AW_MEAN, p, cap, g.bw.bytes, nslots);
    Carve k(p, cap, g.aw.bytes);
    g.fac = k.take<double>((size_t)B * sfb_keep_doubles(n16, sfb_nbr(halfwidth), sfb_nrb(nrhs)));
    g.T = k.take<double>((size_t)B * nrhs * c->npad);
    g.M = k.take<double>((size_t)B * nrhs * nrhs);
    if (want_cov) {
        g.sigma = k.take<double>((size_t)B * n16 * g.bw.ldb);
        g.M2 = k.take<double>((size_t)B * nrhs * nrhs);
        g.stage2 = k.take<double>((size_t)B * nrhs * c->npad);
        g.part = k.take<double>(sf_cov_grad_work_doubles(c->n, mdl->has_global, mdl->n_local, B));
    }
    g.bytes = sf_align_up(k.off, 256);
    return g;
}

// sf_diagnose_banded_batch with k = nrhs right-hand sides, behind the Work of the same call: the band solver's buffers
// (carve_band), the applied layout (carve_applied: the staging area [B][k][npad] that ends up holding alpha, lnl, info and, with
// want_comp, yv), then the pieces of carve_band_grad for a sweep over k + m rows: fac, T: [B][k + m][npad] = Bd^-1 [R^T, Y^T],
// M: [B][(k + m) k].  Then what caller right-hand sides need (the size query does not know whether there are any): rhs:
// [B][k + m][npad], the sweep's rows [R; Y]; gram: [B][(k + m)^2]; zero: [B] zeros (the squared distance of a call that has no
// residual of its own).  Behind them, with want_cinv_diag (NULL otherwise), sigma: the band of Bd^-1, [B][n16][bw.ldb]; M2:
// [B][(k + m) m]; vs: [B][m][npad], the columns of Vs
struct BandDiagWork {
    BandWork bw;
    AppliedWork aw;
    double *fac, *T, *M;
    double *rhs, *gram, *zero;
    double *sigma, *M2, *vs;
    size_t bytes;
};
static BandDiagWork carve_band_diag(const sf_ctx* c, const sf_model_desc* mdl, int B, int halfwidth, int k, bool want_cinv_diag,
                                    bool want_comp, void* p, size_t cap, size_t base_bytes) {
    BandDiagWork g{};
    const int nin = k + c->m, n16 = (c->n + 15) / 16 * 16;
    g.bw = carve_band(c, B, halfwidth, p, cap, base_bytes);
    g.aw = carve_applied(c, mdl, B, k, want_comp ? AW_YV : 0, p, cap, g.bw.bytes);
    Carve w(p, cap, g.aw.bytes);
    g.fac = w.take<double>((size_t)B * sfb_keep_doubles(n16, sfb_nbr(halfwidth), sfb_nrb(nin)));
    g.T = w.take<double>((size_t)B * nin * c->npad);
    g.M = w.take<double>((size_t)B * nin * k);
    g.rhs = w.take<double>((size_t)B * nin * c->npad);
    g.gram = w.take<double>((size_t)B * nin * nin);
    g.zero = w.take<double>((size_t)B);
    if (want_cinv_diag) {
        g.sigma = w.take<double>((size_t)B * n16 * g.bw.ldb);
        g.M2 = w.take<double>((size_t)B * nin * c->m);
        g.vs = w.take<double>((size_t)B * c->m * c->npad);
    }
    g.bytes = sf_align_up(w.off, 256);
    return g;
}

// sf_local_scan_banded_batch, behind the Work of the same call: carve_band_diag's layout for one right-hand side (the walker's
// own residual) with want_cinv_diag at the half-width the head runs at, then what AW_LOCAL_SCAN holds: patch, two ints per
// candidate, and wband, [B][blocks][2 reach + 1][64][64] doubles with reach = min(blocks - 1, 3) (sf_local_scan_banded_doubles)
// -- linear in n
struct BandLocalScanWork {
    BandDiagWork d;
    int* patch;
    double* wband;
    size_t bytes;
};
static BandLocalScanWork carve_band_local_scan(const sf_ctx* c, const sf_model_desc* mdl, int B, int halfwidth, int ncand, void* p,
                                               size_t cap, size_t base_bytes) {
    BandLocalScanWork g{};
    g.d = carve_band_diag(c, mdl, B, halfwidth, 1, true, false, p, cap, base_bytes);
    Carve k(p, cap, g.d.bytes);
    g.patch = k.take<int>(2 * (size_t)ncand);
    g.wband = k.take<double>(sf_local_scan_banded_doubles(c->n, B));
    g.bytes = sf_align_up(k.off, 256);
    return g;
}

// sf_fisher_banded_mean_batch with p = nslots columns, behind the Work of the same call: the band solver's buffers (carve_band;
// its gram takes the leading (1 + m)^2 block for the capacitance step), the applied layout with nin = 1 + m + p rows per walker
// (carve_applied with AW_MEAN: the staging area holds the sweep's rows [r; Y; J]; lnl, info, xs and the tangents' buffers), then
// gram: [B][nin^2], the sweep's Gram matrices, and twist: the two half sweeps' workspace for nin rows
struct BandFisherWork {
    BandWork bw;
    AppliedWork aw;
    double *gram, *twist;
    size_t bytes;
};
static BandFisherWork carve_band_fisher(const sf_ctx* c, const sf_model_desc* mdl, int B, int halfwidth, int nslots, void* p,
                                        size_t cap, size_t base_bytes) {
    BandFisherWork g{};
    const int nin = 1 + c->m + nslots;
    g.bw = carve_band(c, B, halfwidth, p, cap, base_bytes);
    g.aw = carve_applied(c, mdl, B, nin, AW_MEAN, p, cap, g.bw.bytes, nslots);
    Carve k(p, cap, g.aw.bytes);
    g.gram = k.take<double>((size_t)B * nin * nin);
    g.twist = k.take<double>(sfb_twist_carve(nullptr, halfwidth, nin, B).doubles);
    g.bytes = sf_align_up(k.off, 256);
    return g;
}

// ------------------------------------------------------------------- multi-order gradient
// (sf_loglike_multi_grad_batch_md; behind the Work of the same call: base_bytes = its size)  Rows are laid out with the
// group's common npad (L.npad), not an order's own.  For all U units: the staging area, nrhs right-hand sides of npad doubles
// per unit -- nrhs = 1 + m if any segment asks for mean slots, else 1 -- so that one launch applies the factor to a whole
// chunk; then, if any segment asks for covariance slots, cinv_diag (npad per unit) and winv (the inverse's scratch, per unit).
// Then per segment, in segment order, the per-unit data of the parts it asks for, as carve_applied lays them out for a
// single-order call (AW_MEAN with the order's own n: xs, fin, mpart, dcoef, kdot, mudot, zdot; AW_PART: part) and, for a
// segment with mean slots and vsini, coef: the walkers' spline coefficients (in a multi-order call the Work's are one set per
// lane, which the lane's next segment overwrites before the contraction reads them).  seg[i].stage / cinv_diag / winv point at
// the segment's units in the shared arrays.
struct MultiGradWork {
    int nrhs;
    bool any_cov;
    double *stage, *cinv_diag, *winv;
    std::vector<AppliedWork> seg;
    size_t bytes;
};
static MultiGradWork carve_multi_grad(const sf_segment* segs, int nseg, const sf_model_desc* const* models,
                                      const sf_grad_request* reqs, const Layout& L, int U, void* p, size_t cap, size_t base_bytes) {
    Carve k(p, cap, base_bytes);
    MultiGradWork g{};
    bool any_mean = false;
    for (int i = 0; i < nseg; ++i) any_mean |= reqs[i].n_mean_slots > 0, g.any_cov |= reqs[i].want_cov != 0;
    g.nrhs = any_mean ? 1 + L.m : 1;
    const size_t npad = (size_t)L.npad, winv1 = sf_chol_inverse_work_doubles(L.npad, 1);
    g.stage = k.take<double>((size_t)U * g.nrhs * npad);
    if (g.any_cov) {
        g.cinv_diag = k.take<double>((size_t)U * npad);
        g.winv = k.take<double>((size_t)U * winv1);
    }
    g.seg.assign(nseg, AppliedWork{});
    size_t u0 = 0;
    for (int i = 0; i < nseg; ++i) {
        const sf_ctx* c = segs[i].ctx;
        const sf_model_desc* mdl = models[i];
        const size_t B = (size_t)segs[i].B;
        const int nslots = reqs[i].n_mean_slots;
        AppliedWork& w = g.seg[i];
        w.stage = g.stage ? g.stage + u0 * g.nrhs * npad : nullptr;
        if (g.any_cov) {
            w.cinv_diag = g.cinv_diag ? g.cinv_diag + u0 * npad : nullptr;
            w.winv = g.winv ? g.winv + u0 * winv1 : nullptr;
        }
        if (nslots > 0) {
            w.xs = k.take<double>(B * c->m * c->n);
            w.fin = k.take<double>(B * sf_mean_fin_doubles(c->m));
            w.mpart = k.take<double>(sf_mean_grad_part_doubles(c->n, nslots, (int)B));
            if (mdl->has_vsini) {
                w.dcoef = k.take<double>(B * c->nf * c->rows);
                w.coef = k.take<double>(B * c->nf * c->rows);
            }
            const size_t ng = (size_t)(nslots < c->P ? nslots : c->P), mM = (size_t)c->m * c->M;
            w.kdot = k.take<double>(ng * B * mM);
            w.mudot = k.take<double>(ng * B * c->m);
            w.zdot = k.take<double>(ng * B * mM * c->m);
        }
        if (reqs[i].want_cov) w.part = k.take<double>(sf_cov_grad_work_doubles(c->n, mdl->has_global, mdl->n_local, (int)B));
        u0 += B;
    }
    g.bytes = sf_align_up(k.off, 256);
    return g;
}

// ------------------------------------------------------------------- multi-order gradient on the band solver
// (sf_loglike_banded_multi_grad_batch_md; behind the Work of the same call, which has no matrices: base_bytes = its size)  One
// common frame for all U units: n16 rows of the sweep (the group's largest order rounded up to whole blocks), rows of npad
// doubles (L.npad), the half-width `halfwidth` (the largest of the call) and its ldb.  For all U units, as carve_band and
// carve_band_grad lay them out for one order: band [U][n16][ldb], gram, logdet_band, gtab, the staging area [U][1 + m][npad],
// fac (the kept factor of a sweep over n16 rows), T, M; with covariance slots in any segment sigma [U][n16][ldb], M2, stage2.
// Then per segment, in segment order, the per-unit data of the parts it asks for with the order's own n (AW_MEAN: xs, fin,
// mpart, dcoef, kdot, mudot, zdot; part) and, for a segment with mean slots and vsini, coef, for the reason carve_multi_grad
// gives.  seg[i].stage points at the segment's units in the shared staging area.
// what the multi-order calls on the band solver share: the frame, the band, the sweep's outputs and the segments' own data
struct BandMultiWork {
    int n16, halfwidth, ldb;
    double *band, *gram, *logdet_band, *gtab;
    std::vector<AppliedWork> seg;
    size_t bytes;
};
struct BandMultiGradWork : BandMultiWork {
    int nrhs;
    bool any_cov;
    double *stage, *fac, *T, *M, *sigma, *M2, *stage2;
    size_t sfac;  // doubles of one unit's kept factor
};
static BandMultiGradWork carve_band_multi_grad(const sf_segment* segs, int nseg, const sf_model_desc* const* models,
                                               const sf_grad_request* reqs, const Layout& L, int n16, int halfwidth, int U, void* p,
                                               size_t cap, size_t base_bytes) {
    Carve k(p, cap, base_bytes);
    BandMultiGradWork g{};
    for (int i = 0; i < nseg; ++i) g.any_cov |= reqs[i].want_cov != 0;
    g.nrhs = 1 + L.m, g.n16 = n16, g.halfwidth = halfwidth, g.ldb = (halfwidth + 2) & ~1;
    g.sfac = sfb_keep_doubles(n16, sfb_nbr(halfwidth), sfb_nrb(g.nrhs));
    const size_t u = (size_t)U, npad = (size_t)L.npad, ng = (size_t)g.nrhs * g.nrhs, unit = (size_t)g.nrhs * npad;
    g.band = k.take<double>(u * n16 * g.ldb);
    g.gram = k.take<double>(u * ng);
    g.logdet_band = k.take<double>(u);
    g.gtab = k.take<double>(u * (g.ldb + 2));
    g.stage = k.take<double>(u * unit);
    g.fac = k.take<double>(u * g.sfac);
    g.T = k.take<double>(u * unit);
    g.M = k.take<double>(u * ng);
    if (g.any_cov) {
        g.sigma = k.take<double>(u * n16 * g.ldb);
        g.M2 = k.take<double>(u * ng);
        g.stage2 = k.take<double>(u * unit);
    }
    g.seg.assign(nseg, AppliedWork{});
    size_t u0 = 0;
    for (int i = 0; i < nseg; ++i) {
        const sf_ctx* c = segs[i].ctx;
        const sf_model_desc* mdl = models[i];
        const size_t B = (size_t)segs[i].B;
        const int nslots = reqs[i].n_mean_slots;
        AppliedWork& w = g.seg[i];
        w.stage = g.stage ? g.stage + u0 * unit : nullptr;
        if (nslots > 0) {
            w.xs = k.take<double>(B * c->m * c->n);
            w.fin = k.take<double>(B * sf_mean_fin_doubles(c->m));
            w.mpart = k.take<double>(sf_mean_grad_part_doubles(c->n, nslots, (int)B));
            if (mdl->has_vsini) {
                w.dcoef = k.take<double>(B * c->nf * c->rows);
                w.coef = k.take<double>(B * c->nf * c->rows);
            }
            const size_t ngrid = (size_t)(nslots < c->P ? nslots : c->P), mM = (size_t)c->m * c->M;
            w.kdot = k.take<double>(ngrid * B * mM);
            w.mudot = k.take<double>(ngrid * B * c->m);
            w.zdot = k.take<double>(ngrid * B * mM * c->m);
        }
        if (reqs[i].want_cov) w.part = k.take<double>(sf_cov_grad_work_doubles(c->n, mdl->has_global, mdl->n_local, (int)B));
        u0 += B;
    }
    g.bytes = sf_align_up(k.off, 256);
    return g;
}

// ------------------------------------------------------------------- multi-order Fisher information on the band solver
// (sf_fisher_banded_multi_batch_md; behind the Work of the same call, which has no matrices: base_bytes = its size)  The common
// frame of carve_band_multi_grad with nin = 1 + m + pmax rows per unit, pmax the largest column count of a segment.  For all U
// units, as carve_band and carve_band_fisher lay them out for one order: band [U][n16][ldb], lead [U][(1 + m)^2] (the Gram
// matrices' leading blocks, for the capacitance step), logdet_band, gtab, buf [U][nin][npad] (the sweep's rows [r; Y; J; 0]),
// gram [U][nin^2], twist (the two half sweeps' workspace for nin rows and U units; the chunks run one after the other and
// share it) and fcomp [U][pmax^2], the compact blocks of k_fisher_band.  Then per segment, in segment order, what the tangent
// columns read per unit with the order's own n: xs, dcoef (vsini), kdot, mudot.  (No coef of its own: the columns are written on
// the segment's lane, behind its chain, before the lane's next segment overwrites the Work's.)
struct BandMultiFisherWork : BandMultiWork {
    int nin, pmax;
    double *lead, *buf, *twist, *fcomp;
};
static BandMultiFisherWork carve_band_multi_fisher(const sf_segment* segs, int nseg, const sf_model_desc* const* models,
                                                   const sf_grad_request* reqs, const Layout& L, int n16, int halfwidth, int pmax, int U,
                                                   void* p, size_t cap, size_t base_bytes) {
    Carve k(p, cap, base_bytes);
    BandMultiFisherWork g{};
    g.pmax = pmax, g.nin = 1 + L.m + pmax, g.n16 = n16, g.halfwidth = halfwidth, g.ldb = (halfwidth + 2) & ~1;
    const size_t u = (size_t)U, npad = (size_t)L.npad, nl = (size_t)(1 + L.m) * (1 + L.m), ng = (size_t)g.nin * g.nin;
    g.band = k.take<double>(u * n16 * g.ldb);
    g.lead = k.take<double>(u * nl);
    g.logdet_band = k.take<double>(u);
    g.gtab = k.take<double>(u * (g.ldb + 2));
    g.buf = k.take<double>(u * g.nin * npad);
    g.gram = k.take<double>(u * ng);
    g.twist = k.take<double>(sfb_twist_carve(nullptr, halfwidth, g.nin, U).doubles);
    g.fcomp = k.take<double>(u * pmax * pmax);
    g.seg.assign(nseg, AppliedWork{});
    size_t u0 = 0;
    for (int i = 0; i < nseg; ++i) {
        const sf_ctx* c = segs[i].ctx;
        const size_t B = (size_t)segs[i].B;
        const int nslots = reqs[i].n_mean_slots;
        AppliedWork& w = g.seg[i];
        w.stage = g.buf ? g.buf + u0 * g.nin * npad : nullptr;
        w.xs = k.take<double>(B * c->m * c->n);
        if (models[i]->has_vsini) w.dcoef = k.take<double>(B * c->nf * c->rows);
        const size_t ngrid = (size_t)(nslots < c->P ? nslots : c->P), mM = (size_t)c->m * c->M;
        w.kdot = k.take<double>(ngrid * B * mM);
        w.mudot = k.take<double>(ngrid * B * c->m);
        u0 += B;
    }
    g.bytes = sf_align_up(k.off, 256);
    return g;
}

// ------------------------------------------------------------------- multi-order score scan on the band solver
// (sf_local_scan_banded_multi_batch_md; behind the Work of the same call, which has no matrices: base_bytes = its size)  The common
// frame of carve_band_multi_grad at the window's widest half-width for 1 + m rows.  For all U units, as carve_band and
// carve_band_diag lay them out for one order and one right-hand side (the walker's own residual): band [U][n16][ldb] (filled
// entry by entry: no table per diagonal), gram [U][(1 + m)^2], logdet_band, the staging area [U][npad] that ends up holding alpha,
// fac (the kept factor of a sweep over n16 rows), T [U][1 + m][npad], M [U][1 + m], sigma [U][n16][ldb], M2 [U][(1 + m) m] and vs
// [U][m][npad].  Then ONE patch list and ONE set of tiles of W for the whole call, sized for the segment that needs the most (2
// ints per candidate; sf_local_scan_banded_doubles of its n and B): the segments' scans run one after the other on the caller's
// stream, and every scan writes both before it reads them.
struct BandMultiScanWork : BandMultiWork {
    int nrhs;
    double *stage, *fac, *T, *M, *sigma, *M2, *vs;
    size_t sfac;  // doubles of one unit's kept factor
    int* patch;
    double* wband;
};
static BandMultiScanWork carve_band_multi_scan(const sf_segment* segs, int nseg, const int* h_cand_ptr, const Layout& L, int n16,
                                               int halfwidth, int U, void* p, size_t cap, size_t base_bytes) {
    Carve k(p, cap, base_bytes);
    BandMultiScanWork g{};
    g.nrhs = 1 + L.m, g.n16 = n16, g.halfwidth = halfwidth, g.ldb = (halfwidth + 2) & ~1;
    g.sfac = sfb_keep_doubles(n16, sfb_nbr(halfwidth), sfb_nrb(g.nrhs));
    const size_t u = (size_t)U, npad = (size_t)L.npad, ng = (size_t)g.nrhs * g.nrhs;
    g.band = k.take<double>(u * n16 * g.ldb);
    g.gram = k.take<double>(u * ng);
    g.logdet_band = k.take<double>(u);
    g.stage = k.take<double>(u * npad);
    g.fac = k.take<double>(u * g.sfac);
    g.T = k.take<double>(u * g.nrhs * npad);
    g.M = k.take<double>(u * g.nrhs);
    g.sigma = k.take<double>(u * n16 * g.ldb);
    g.M2 = k.take<double>(u * g.nrhs * L.m);
    g.vs = k.take<double>(u * L.m * npad);
    size_t ncand = 0, tiles = 0;
    for (int i = 0; i < nseg; ++i) {
        ncand = std::max(ncand, (size_t)(h_cand_ptr[i + 1] - h_cand_ptr[i]));
        tiles = std::max(tiles, sf_local_scan_banded_doubles(segs[i].ctx->n, segs[i].B));
    }
    g.patch = k.take<int>(2 * ncand);
    g.wband = k.take<double>(tiles);
    g.bytes = sf_align_up(k.off, 256);
    return g;
}

// ------------------------------------------------------------------- context-free workspaces
// sf_potri_diag_batch: the transposed inverses of the 64 x 64 diagonal blocks, [batch][n / 64][64][64]; sf_potri_blocks_batch
// (with_diag): the same, then the diagonal of the inverse ([batch][n]: the inverse's launch writes it)
struct PotriWork {
    double *winv, *diag;
    size_t bytes;
};
static PotriWork carve_potri(int n, int batch, void* p, size_t cap, bool with_diag = false) {
    Carve k(p, cap);
    PotriWork w{};
    w.winv = k.take<double>(sf_chol_inverse_work_doubles(n, batch));
    if (with_diag) w.diag = k.take<double>((size_t)n * batch);
    w.bytes = sf_align_up(k.off, 256);
    return w;
}
// sf_potrf_batch / sf_logdet_sqmah_batch: z scratch of the stand-alone solve + the transposed leaf factor read by the panel solves
struct PotrfWork {
    double *z, *ltbuf;
    size_t bytes;
};
static PotrfWork carve_potrf(int n, int batch, void* p, size_t cap) {
    Carve k(p, cap);
    PotrfWork w;
    w.z = k.take<double>((size_t)n * batch);
    w.ltbuf = k.take<double>(sf_potrf_work_doubles(n, batch));
    w.bytes = sf_align_up(k.off, 256) + 256;  // (slack the size query has always included)
    return w;
}
// the broadening free functions: twiddles, then the scratch of a transform that does not fit the LDS
struct FftWork {
    double* tw;
    double2* scratch;
    size_t bytes;
};
static FftWork carve_fft(int rows, int nf, void* p, size_t cap) {
    Carve k(p, cap);
    FftWork w;
    const size_t fb = sf_fft_scratch_bytes(rows, nf);
    w.tw = k.take<double>((size_t)nf);
    w.scratch = k.take<double2>(fb / sizeof(double2));
    if (!fb) w.scratch = nullptr;
    w.bytes = k.off + 256;  // (slack the size query has always included)
    return w;
}
// sf_resample: knots, Lf, Uf, rdiag, coefficient rows
struct ResampleWork {
    double *t, *Lf, *Uf, *rdiag, *coef;
    size_t bytes;
};
static ResampleWork carve_resample(int n, int rows, void* p, size_t cap) {
    Carve k(p, cap);
    ResampleWork w;
    w.t = k.take<double>((size_t)n + 6);
    w.Lf = k.take<double>((size_t)n * SF_KB);
    w.Uf = k.take<double>((size_t)n * SF_KB);
    w.rdiag = k.take<double>((size_t)n);
    w.coef = k.take<double>((size_t)n * rows);
    w.bytes = sf_align_up(k.off, 256) + 1024;  // (slack the size query has always included)
    return w;
}
// The training objective for B hyper-parameter rows: the B matrices (npad = m M rounded up to the Cholesky leaf, row stride
// npad + 16 as Emulator.log_likelihood lays its one matrix out), the B x npad right-hand sides, logdet / sqmah / the
// factorisation's info, then the workspace of sf_potrf_batch (carve_potrf).  With grad_P > 0 (grid axes:
// sf_emulator_loglike_grad_batch), behind all that and so at the same offsets: alpha = v11^-1 w_hat (B x npad), the scratch
// of the inverse's launch and the row of the inverse's diagonal it writes (carve_potri; the gradient does not read the row),
// and the gradient's partial sums, one double per (matrix, 64-row block, slot).
struct EmuTrainWork {
    int npad, lda;
    int64_t stride;
    double *A, *R, *logdet, *sqmah;
    int* info_c;
    char* potrf;
    double *alpha, *winv, *cinv_diag, *part;
    size_t potrf_bytes, bytes;
};
static EmuTrainWork carve_emu_train(int M, int m, int B, void* p, size_t cap, int grad_P = 0) {
    EmuTrainWork w = {};
    if (M <= 0 || m <= 0 || B <= 0 || (int64_t)m * M > (1 << 30)) return w;
    w.npad = (m * M + SF_LEAF - 1) / SF_LEAF * SF_LEAF;
    w.lda = w.npad + 16;
    w.stride = (int64_t)w.npad * w.lda;
    const size_t b = (size_t)B;
    Carve k(p, cap);
    w.A = k.take<double>(b * (size_t)w.stride);
    w.R = k.take<double>(b * w.npad);
    w.logdet = k.take<double>(b);
    w.sqmah = k.take<double>(b);
    w.info_c = k.take<int>(b);
    w.potrf_bytes = carve_potrf(w.npad, B, nullptr, 0).bytes;
    w.potrf = k.take<char>(w.potrf_bytes);
    if (grad_P > 0) {
        w.alpha = k.take<double>(b * w.npad);
        const PotriWork pw = carve_potri(w.npad, B, nullptr, 0, true);
        char* potri = k.take<char>(pw.bytes);
        const PotriWork pi = carve_potri(w.npad, B, potri, pw.bytes, true);
        w.winv = pi.winv, w.cinv_diag = pi.diag;
        w.part = k.take<double>(sf_emu_grad_work_doubles(M, grad_P, m, B));
    }
    w.bytes = k.off;
    return w;
}
