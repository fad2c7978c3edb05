// The launch sequences on the panel kernels: the narrow step (k_chol_panel) and the wide step (k_chol_panel_w) as launches,
// the diagonal step, one narrow step of a chain and two slab groups, and the fused (sf_launch_potrf_v2) and wide
// (sf_launch_potrf_v3) sequences built from them.  Used by sf_launch_potrf; the band driver borrows the step helpers.
#pragma once
#include "sf_chol_host.h"
#include "sf_chol_diag.h"
#include "sf_chol_panel.h"
#include "sf_chol_wide.h"

// The fused sequences work in the frame of sf_potrf_front_pad (sf_launch_potrf shifts it): A / rhs point fp (lda + 1) / fp
// elements before the data and n counts the fp virtual leading rows too (the scratch layout is sized with the real n).
static int sf_check_front_pad(int fp, int n) {
    if (fp != 0 && (fp != 64 || n % GT != 64)) {
        sf_set_error("potrf: front pad %d does not fit n = %d", fp, n);
        return SF_EINVAL;
    }
    return SF_OK;
}

// The first slab's updated diagonal tile is parked in the scratch T (for the next D step) instead of stored in place
template <class Args>
static void sf_park(Args& g, const sf_potrf_scratch& ws) {
    g.Sout = ws.T;
    g.sS = ws.sT;
    g.ldS = SF_LDT;
}
// Rows of nslab slabs of 128 rows, the first at row0, `step` slabs apart, in a matrix of order n (the last slab may be shorter)
static double sf_slab_rows(int n, int row0, int nslab, int step) {
    double rows = 0.0;
    for (int i = 0; i < nslab; ++i) {
        const int r0 = row0 + i * step * GT;
        rows += (n - r0 < GT) ? n - r0 : GT;
    }
    return rows;
}
static int sf_check_grid(long long nblk) {
    if (nblk > 0x7fffffffLL) {
        sf_set_error("panel grid too large");
        return SF_EINVAL;
    }
    return SF_OK;
}

// split-K factor of a narrow step of nblk workgroups (1: not split)
static int sf_panel_split(int k0, int pw, int fp, long long nblk) {
    return pw > 0 ? sf_split_policy(nblk, (k0 > fp ? k0 - fp : 0) / GK) : 1;
}
// One narrow step (k_chol_panel) of the fused and the wide sequence: panel [k0, k0 + pw) for nslab slabs of every matrix, the
// first at row0, `step` slabs apart.  g: the fields that stay the same over the factorisation (sf_panel_frame).  to_scratch:
// the chain's step -- the first slab's updated diagonal tile is parked in the scratch T, the workgroups run at raised wave
// priority.  A split step parks its partial sums in region `region` of `part`; phase 0 launches the whole step, 1 / 2 only
// the split-K partial sums / only what follows them.
static int sf_panel_step(sf_panel_args g, const sf_potrf_scratch& ws, int k0, int pw, int row0, int nslab, int step, const double* Wt,
                         bool to_scratch, hipStream_t st, int region, int phase) {
    const int n = g.n, fp = g.fp, batch = ws.batch;
    g.k0 = k0;
    g.pw = pw;
    g.row0 = row0;
    g.nslab = nslab;
    g.slab_step = step;
    g.Wt = Wt;
    g.sW = ws.sW;
    if (to_scratch) {
        sf_park(g, ws);
        g.prio = 1;
    }
    const long long nblk = (long long)nslab * batch;
    SF_TRY(sf_check_grid(nblk));
    // algorithmic flops: update 2 k0 rows pw, solve rows pw^2, symmetric rank-pw update of the lower tiles
    const double rows = sf_slab_rows(n, row0, nslab, step);
    const double flops_main = 2.0 * (k0 > fp ? k0 - fp : 0) * rows * pw * batch;
    const double flops_epi = (rows * pw * (double)pw + (double)GT * rows * pw) * batch;
    const int nk = (k0 > fp ? k0 - fp : 0) / GK;
    const int S = sf_panel_split(k0, pw, fp, nblk);
    void* tok;  // (every kernel launch is one profiled launch: what rocprofv3 --stats counts)
    if (S > 1) {
        g.ksplit = S;
        g.kchunk = (nk + S - 1) / S;
        g.part = ws.part + (size_t)region * sf_split_region_tiles() * (GT * GT);
        if (phase != 2) {
            sf_prof_gemm_begin(st, flops_main, &tok);
            hipLaunchKernelGGL((k_chol_panel<false, 1>), dim3((unsigned)(nblk * S)), dim3(512), 0, st, g);
            sf_prof_gemm_end(tok);
        }
        if (phase != 1) {
            sf_prof_gemm_begin(st, flops_epi, &tok);
            if (g.rhs)
                hipLaunchKernelGGL((k_chol_panel<true, 2>), dim3((unsigned)nblk), dim3(512), 0, st, g);
            else
                hipLaunchKernelGGL((k_chol_panel<false, 2>), dim3((unsigned)nblk), dim3(512), 0, st, g);
            sf_prof_gemm_end(tok);
        }
    } else {
        sf_prof_gemm_begin(st, flops_main + flops_epi, &tok);
        if (g.rhs)
            hipLaunchKernelGGL((k_chol_panel<true, 0>), dim3((unsigned)nblk), dim3(512), 0, st, g);
        else
            hipLaunchKernelGGL((k_chol_panel<false, 0>), dim3((unsigned)nblk), dim3(512), 0, st, g);
        sf_prof_gemm_end(tok);
    }
    SF_LAUNCH_CHECK();
    return SF_OK;
}

// Tuning builds (SF_WIDE_STAMPS): 100 MHz wall-clock stamps of the phases of one workgroup per wide launch, up to 64
// launches of 16 stamps in host memory, with the (panel, slab count) each belongs to.  Empty in release builds.
struct sf_wide_stamps {
#ifdef SF_TUNING
    long long* t = nullptr;
    int n = 0, k[64];
#endif
};
#ifdef SF_TUNING
static int sf_wide_stamps_begin(sf_wide_stamps& w) {
    if (SF_TUNE_FLAG("SF_WIDE_STAMPS")) {
        SF_HIP(hipHostMalloc((void**)&w.t, sizeof(long long) * 16 * 64));
        for (int i = 0; i < 16 * 64; ++i) w.t[i] = 0;
    }
    return SF_OK;
}
static void sf_wide_stamps_report(sf_wide_stamps& w, hipStream_t s) {
    if (!w.t) return;  // (synchronises: phases of one workgroup per wide launch, us)
    (void)hipStreamSynchronize(s);
    fprintf(stderr, "wide launches, workgroup grid/2: k nslab | prologue | K loop | solve 1 | 2b | solve 2 | store + rhs | S load + step 4 | S store + drain | total (us)\n");
    for (int i = 0; i < w.n; ++i) {
        const long long* t = w.t + 16 * i;
        fprintf(stderr, "%2d %2d |", w.k[i] / 1000, w.k[i] % 1000);
        const int seg[8][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 4}, {4, 5}, {5, 6}, {6, 7}, {7, 8}};
        for (auto& sg : seg) fprintf(stderr, " %7.1f |", (t[sg[1]] - t[sg[0]]) / 100.0);
        fprintf(stderr, " %7.1f\n", (t[8] - t[0]) / 100.0);
    }
    // the interval 6 -> 7 of the same launches, per half (panel k, panel k + 1) of step 4
    fprintf(stderr, "step 4 of the same launches: k nslab | half 0: dump | wait for S | MFMA | half 1: dump | wait for S | MFMA (us)\n");
    for (int i = 0; i < w.n; ++i) {
        const long long* t = w.t + 16 * i;
        fprintf(stderr, "%2d %2d |", w.k[i] / 1000, w.k[i] % 1000);
        const int seg[6][2] = {{6, 9}, {9, 10}, {10, 11}, {11, 12}, {12, 13}, {13, 14}};
        for (auto& sg : seg) fprintf(stderr, " %7.2f |", (t[sg[1]] - t[sg[0]]) / 100.0);
        fprintf(stderr, "\n");
    }
    (void)hipHostFree(w.t);
}
#else
static int sf_wide_stamps_begin(sf_wide_stamps&) { return SF_OK; }
static void sf_wide_stamps_report(sf_wide_stamps&, hipStream_t) {}
#endif

// One wide step (k_chol_panel_w): the pair of panels k, k + 1 for nslab slabs of every matrix, the first slab slab0, `step`
// slabs apart.  g: the fields that stay the same over the factorisation (sf_panel_frame).  park: the first slab's updated
// diagonal tile goes to the scratch T.
static int sf_panel_step_w(sf_panelw_args g, const sf_potrf_scratch& ws, int k, int slab0, int nslab, int step, bool park, hipStream_t st,
                           sf_wide_stamps& stamps) {
    const int n = g.n, fp = g.fp, batch = ws.batch;
    g.k0 = k * GT;
    g.row0 = slab0 * GT;
    g.nslab = nslab;
    g.slab_step = step;
    g.Wt0 = ws.Wslot(k);
    g.Wt1 = ws.Wslot(k + 1);
    g.sW = ws.sW;
    if (park) sf_park(g, ws);
    const long long nblk = (long long)nslab * batch;
    SF_TRY(sf_check_grid(nblk));
#ifdef SF_TUNING
    if (stamps.t && stamps.n < 64) {
        stamps.k[stamps.n] = k * 1000 + nslab;
        g.stamps = stamps.t + 16 * stamps.n++;
    }
#endif
    const double rows = sf_slab_rows(n, g.row0, nslab, step);
    // algorithmic flops of the two panel steps it replaces: update 2 k0 rows 128 (+ 128 more K for the second panel),
    // solves rows 128^2 each, symmetric rank-128 updates of the lower tiles
    const double kk = g.k0 > fp ? g.k0 - fp : 0;
    const double flops = (2.0 * kk * rows * GT + 2.0 * (kk + GT) * rows * GT + 2.0 * (rows * GT * (double)GT + (double)GT * rows * GT)) * batch;
    void* tok;
    sf_prof_gemm_begin(st, flops, &tok);
    if (g.rhs)
        hipLaunchKernelGGL(k_chol_panel_w<true>, dim3((unsigned)nblk), dim3(1024), SF_PANELW_LDS, st, g);
    else
        hipLaunchKernelGGL(k_chol_panel_w<false>, dim3((unsigned)nblk), dim3(1024), SF_PANELW_LDS, st, g);
    sf_prof_gemm_end(tok);
    SF_LAUNCH_CHECK();
    return SF_OK;
}

// D(k): k_diag_lds on the diagonal tile of panel k (parked in the scratch T) of a matrix of order n in the frame fp: L_kk
// in place, L_kk^-1 to Wt, z_k into rhs (NULL: none)
static int sf_diag_step(const sf_potrf_scratch& ws, double* A, int lda, int64_t stride, double* rhs, int ldr, int* info, int n, int k,
                        double* Wt, int fp, hipStream_t st) {
    const int k0 = k * GT;
    const int pw = (n - k0 < GT) ? n - k0 : GT;
    return sf_launch_diag128(ws.T, ws.sT, pw, info, k0 - fp, rhs ? rhs + k0 : nullptr, ldr, A + (int64_t)k0 * lda + k0, lda, stride, Wt,
                             ws.sW, ws.batch, st, k == 0 ? fp : 0);
}

// One narrow step of a chain stream c and two slab groups (slab i on gs[i & 1]): D(k) on the chain into the inverse-tile buffer
// Wt; top(k), the slab of the next diagonal tile, on the chain after the last launch of that slab's group (last[]); rest(k),
// the slabs k+2 .. of either group, after D(k).  The caller enqueues what D(k) must wait for in front and keeps the books
// behind: ev holds the events recorded here (NULL where a group has no slab left; all NULL for the last panel: D(k) alone).
// e_top non-NULL: the fused sequence's own top(k) -- when the step is split its partial sums run BESIDE D(k) on the stream of
// that slab's group, after *e_top (the end of top(k-1): row k's columns of panel k-1, the partial-sum region), and the end of
// top(k) is recorded into *e_top.  The wide sequence passes NULL and never took that path: it says which sequence calls, it
// is not a tuning knob.
struct sf_narrow_events {
    hipEvent_t d, rest[2];
};
static int sf_narrow_step(const sf_panel_args& base, const sf_potrf_scratch& ws, sf_exec* ex, int* info, int k, double* Wt, hipStream_t c,
                          const hipStream_t gs[2], const hipEvent_t last[2], hipEvent_t* e_top, sf_narrow_events* ev) {
    const int n = base.n, fp = base.fp, nt = (n + GT - 1) / GT;
    const int k0 = k * GT;
    const int pw = (n - k0 < GT) ? n - k0 : GT;
    *ev = {};
    SF_TRY(sf_diag_step(ws, base.C, base.lda, base.sC, base.rhs, base.ldr, info, n, k, Wt, fp, c));
    if (k + 1 >= nt) return SF_OK;
    SF_TRY(sf_exec_event(ex, &ev->d));
    SF_HIP(hipEventRecord(ev->d, c));
    // top(k).  Its long-K part (split-K partial sums) needs the rows of slabs k and k+1 left of the panel, not D(k): the
    // fused sequence's chain is D(k) | partial sums -> reduce + solve + diagonal tile -> D(k+1).
    const int gk = (k + 1) & 1;
    if (e_top && sf_panel_split(k0, pw, fp, ws.batch) > 1) {
        if (*e_top) SF_HIP(hipStreamWaitEvent(gs[gk], *e_top, 0));
        SF_TRY(sf_panel_step(base, ws, k0, pw, (k + 1) * GT, 1, 1, Wt, true, gs[gk], 0, 1));
        hipEvent_t e_part;
        SF_TRY(sf_exec_event(ex, &e_part));
        SF_HIP(hipEventRecord(e_part, gs[gk]));
        SF_HIP(hipStreamWaitEvent(c, e_part, 0));
        SF_TRY(sf_panel_step(base, ws, k0, pw, (k + 1) * GT, 1, 1, Wt, true, c, 0, 2));
    } else {
        if (last[gk]) SF_HIP(hipStreamWaitEvent(c, last[gk], 0));
        SF_TRY(sf_panel_step(base, ws, k0, pw, (k + 1) * GT, 1, 1, Wt, true, c, 0, 0));
    }
    if (e_top) {
        SF_TRY(sf_exec_event(ex, e_top));
        SF_HIP(hipEventRecord(*e_top, c));
    }
    // rest(k): slabs k+2 .. nt-1 (split-K partial sums in ws.part: region 0 = chain, 1 + g = group g)
    for (int g = 0; g < 2; ++g) {
        const int first = k + 2 + (((k + 2) & 1) != g);
        if (first >= nt) continue;
        const int cnt = (nt - 1 - first) / 2 + 1;
        SF_HIP(hipStreamWaitEvent(gs[g], ev->d, 0));
        SF_TRY(sf_panel_step(base, ws, k0, pw, first * GT, cnt, 2, Wt, false, gs[g], 1 + g, 0));
        SF_TRY(sf_exec_event(ex, &ev->rest[g]));
        SF_HIP(hipEventRecord(ev->rest[g], gs[g]));
    }
    return SF_OK;
}

// Factorisation with the fused panel kernel (default).  Panels of 128 columns; per panel k
//   D(k)      k_diag_lds on the updated diagonal tile (parked in the scratch T): L_kk, L_kk^-1, z_k
//   top(k)    k_chol_panel for the slab of the NEXT diagonal tile (rows k1 .. k1+128): its updated tile goes to T
//   rest(k)   k_chol_panel for all slabs below, as G launches on G streams: slab i belongs to group i mod G
// Lookahead: the chain  D(k) -> [wait group of slab k+1] top(k) -> D(k+1) ...  runs on the side stream;
// group g only needs D(k) (which ran beside rest(k-1)) and its own previous launch (a slab stays in its
// group), so there is no chip-wide barrier between panels: while one group's launch drains its last
// workgroups the other groups keep the CUs full (one launch per panel left 0.25-0.75 of a round of 512
// workgroups idle at every panel boundary).
static int sf_launch_potrf_v2(double* A, int n, int lda, int64_t stride, int* info, const sf_potrf_scratch& ws, double* rhs,
                              int ldr, hipStream_t s, const sf_gen_args* gen, sf_exec* ex, int fp) {
    const int batch = ws.batch;
    SF_HIP(hipMemsetAsync(info, 0, sizeof(int) * (size_t)batch, s));
    SF_TRY(sf_exec_prepare(ex));
    constexpr int G = 2;  // slab groups: group 0 on the caller's stream, group 1 on grp[0]
    hipStream_t c = ex->side;
    const hipStream_t gs[G] = {s, ex->grp[0]};
    SF_TRY(sf_exec_fork(ex, s, {c, gs[1]}));

    const sf_panel_args base = sf_panel_frame<sf_panel_args>(A, n, lda, stride, rhs, ldr, gen, fp);
    const int nt = (n + GT - 1) / GT;
    // diagonal tile 0 goes to the scratch unchanged
    SF_TRY(sf_panel_step(base, ws, 0, 0, 0, 1, 1, nullptr, true, c, 0, 0));
    hipEvent_t e_epi = nullptr;      // end of top(k-1) on the chain
    hipEvent_t e_rest[G] = {};       // last launch of every group
    hipEvent_t e_rest_prev[G] = {};  // ... one panel earlier (their readers of Wt[panel & 1])
    for (int k = 0; k < nt; ++k) {
        // D(k) overwrites the W buffer of panel k-2: every group must be done reading it
        for (int g = 0; g < G; ++g)
            if (e_rest_prev[g]) SF_HIP(hipStreamWaitEvent(c, e_rest_prev[g], 0));
        sf_narrow_events ev;
        SF_TRY(sf_narrow_step(base, ws, ex, info, k, ws.Wbuf(k & 1), c, gs, e_rest, &e_epi, &ev));
        for (int g = 0; g < G; ++g) {
            e_rest_prev[g] = e_rest[g];
            if (ev.rest[g]) e_rest[g] = ev.rest[g];
        }
    }
    // join: the caller's stream continues only after the chain and every group are done
    SF_TRY(sf_exec_join(ex, s, c, {e_rest[1]}));
    return SF_OK;
}

// Factorisation with the WIDE panel kernel: pairs of panels.  Per pair p (panels k = 2p, k + 1; columns [k0, k0 + 256)):
//   chain(p)  on the side stream:  D(k) -> top(k): narrow k_chol_panel for slab k+1 (gives L21, parks tile (k+1, k+1))
//             -> D(k+1);  depends on A(p-1) only
//   A(p)      k_chol_panel_w for the slabs k+2, k+3 (the rows of the NEXT pair's diagonal block; parks tile (k+2, k+2)):
//             one round of workgroups on its own stream, so that chain(p+1) runs beside B(p)
//   B(p)      k_chol_panel_w for the slabs k+4 .. on the caller's stream
// A trailing single panel (odd number of panels) and pairs without rows below them are narrow steps of the chain.
// The four most recent inverse tiles W(k) live in the two 256-row buffers of the narrow sequence (slot k & 3).
// half (test aid, sequence 3): narrow steps from the middle on -- exercises the hand-over on any size.
static int sf_launch_potrf_v3(double* A, int n, int lda, int64_t stride, int* info, const sf_potrf_scratch& ws, double* rhs,
                              int ldr, hipStream_t s, const sf_gen_args* gen, sf_exec* ex, bool half, int fp) {
    const int batch = ws.batch;
    static sf_dev_once attr_once;
    SF_CHECK(sf_lds_limit_once(&attr_once, 160 * 1024, {(const void*)k_chol_panel_w<true>, (const void*)k_chol_panel_w<false>}));
    SF_HIP(hipMemsetAsync(info, 0, sizeof(int) * (size_t)batch, s));
    SF_TRY(sf_exec_prepare(ex));
    // A(p) sits between chain(p) and chain(p+1) anyway: it shares the chain's stream.  A stream of its own made a cfg-2
    // step 3 % slower (48.4 -> 50.0 ms: every additional ACTIVE stream costs dispatch latency on all of them -- the
    // transform chain ahead of the factorisation went from 0.40 to 0.70 ms); at cfg 3, where an A launch is ten rounds of
    // workgroups, a separate stream measured the same (265.1 / 267.0 vs 266.8 / 265.8 ms).
    hipStream_t c = ex->side, xa = ex->side;
    SF_TRY(sf_exec_fork(ex, s, {c, xa, ex->grp[0]}));
    const int nt = (n + GT - 1) / GT;

    const sf_panel_args base = sf_panel_frame<sf_panel_args>(A, n, lda, stride, rhs, ldr, gen, fp);
    const sf_panelw_args wbase = sf_panel_frame<sf_panelw_args>(A, n, lda, stride, rhs, ldr, gen, fp);
    sf_wide_stamps stamps;
    SF_TRY(sf_wide_stamps_begin(stamps));
    auto diag = [&](int k) -> int { return sf_diag_step(ws, A, lda, stride, rhs, ldr, info, n, k, ws.Wslot(k), fp, c); };

    SF_TRY(sf_panel_step(base, ws, 0, 0, 0, 1, 1, nullptr, true, c, 0, 0));  // diagonal tile 0 goes to the scratch unchanged
    // B(p) runs as two interleaved slab groups on two streams (like the narrow sequence): a group's next launch only
    // needs its own previous one, so the last, partly filled round of one group overlaps the other group's work.
    // Group g = slabs of parity g (k even: k+4+g, k+6+g, ...), in the wide pairs and in the narrow tail alike.
    const hipStream_t bs[2] = {s, ex->grp[0]};
    hipEvent_t e_A = nullptr;
    hipEvent_t e_last[2] = {nullptr, nullptr};        // last launch of either group
    std::vector<hipEvent_t> readers[4];               // launches that read W slot j (a D step may only overwrite it after them)
    auto wait_readers = [&](int slot) -> int {
        for (hipEvent_t e : readers[slot]) SF_HIP(hipStreamWaitEvent(c, e, 0));
        readers[slot].clear();
        return SF_OK;
    };
    int k = 0;
    for (; k < nt; k += 2) {
        if (k + 2 >= nt) break;  // no rows below the pair: the narrow loop finishes the diagonal block
        if (half && k >= (nt / 4) * 2 && k > 0) break;  // -> narrow tail from panel k
        // chain(p): needs the tile parked by A(p-1) and the rows of slab k+1 (A(p-1))
        if (e_A) SF_HIP(hipStreamWaitEvent(c, e_A, 0));
        SF_TRY(wait_readers(k & 3));
        SF_TRY(diag(k));
        SF_TRY(sf_panel_step(base, ws, k * GT, GT, (k + 1) * GT, 1, 1, ws.Wslot(k), true, c, 0, 0));  // (rows below the pair exist: panel k is full)
        SF_TRY(wait_readers((k + 1) & 3));
        SF_TRY(diag(k + 1));
        hipEvent_t e_chain;
        SF_TRY(sf_exec_event(ex, &e_chain));
        SF_HIP(hipEventRecord(e_chain, c));
        // A(p): slabs k+2, k+3 -- needs chain(p) and the rows B(p-1) finished (the first slab of either group)
        const int na = (nt - (k + 2) < 2) ? nt - (k + 2) : 2;
        SF_HIP(hipStreamWaitEvent(xa, e_chain, 0));
        for (int g = 0; g < 2; ++g)
            if (e_last[g]) SF_HIP(hipStreamWaitEvent(xa, e_last[g], 0));
        SF_TRY(sf_panel_step_w(wbase, ws, k, k + 2, na, 1, true, xa, stamps));
        SF_TRY(sf_exec_event(ex, &e_A));
        SF_HIP(hipEventRecord(e_A, xa));
        readers[k & 3].push_back(e_A);
        readers[(k + 1) & 3].push_back(e_A);
        // B(p): slabs k+4 .., slab k+4+g, k+6+g, ... in group g
        for (int g = 0; g < 2; ++g) {
            const int first = k + 4 + g;
            if (first >= nt) continue;
            const int cnt = (nt - 1 - first) / 2 + 1;
            SF_HIP(hipStreamWaitEvent(bs[g], e_chain, 0));
            SF_TRY(sf_panel_step_w(wbase, ws, k, first, cnt, 2, false, bs[g], stamps));
            SF_TRY(sf_exec_event(ex, &e_last[g]));
            SF_HIP(hipEventRecord(e_last[g], bs[g]));
            readers[k & 3].push_back(e_last[g]);
            readers[(k + 1) & 3].push_back(e_last[g]);
        }
    }
    // The narrow tail finishes what the pairs leave (a trailing single panel, pairs without rows below them, the last
    // diagonal block), one narrow step per panel.  (The timeline suggested that the last pairs -- few rounds of ~1 ms
    // workgroups, every dependency of the chain costs a round -- would be better off as narrow steps, the measurement says
    // no: cfg 2, wide to the end 49.3 ms, hand-over with 2 / 5 / 8 / 12 rounds left 50.0 / 50.4 / 51.0 / 51.8, narrow 51.5.)
    for (; k < nt; ++k) {
        if (e_A) {  // the tile parked by the last wide A launch, and the rows of its two slabs
            SF_HIP(hipStreamWaitEvent(c, e_A, 0));
            for (int g = 0; g < 2; ++g) SF_HIP(hipStreamWaitEvent(bs[g], e_A, 0));
            e_A = nullptr;
        }
        SF_TRY(wait_readers(k & 3));
        sf_narrow_events ev;
        SF_TRY(sf_narrow_step(base, ws, ex, info, k, ws.Wslot(k), c, bs, e_last, nullptr, &ev));
        for (int g = 0; g < 2; ++g)
            if (ev.rest[g]) {
                e_last[g] = ev.rest[g];
                readers[k & 3].push_back(ev.rest[g]);
            }
    }
    SF_TRY(sf_exec_join(ex, s, c, {e_A, e_last[1]}));
    sf_wide_stamps_report(stamps, s);
    return SF_OK;
}
