// Host-side pieces every launch sequence shares: the scratch layout and its skew, the split-K policy, the frame and
// generator fields of the kernel arguments, fork / join of the executor's streams.  Used by all five launchers.
#pragma once
#include "sf_chol_tile.h"

// The per-matrix scratch strides are skewed by a few hundred bytes: with strides that are multiples of
// 32 KiB every workgroup of the batch touches the same HBM channel / L2 bank at the same time (measured:
// 3.6 us per dependent load in k_diag_mfma before the skew).
#define SF_TSKEW 40
// Split-K policy of the fused factorisation: a launch of `wgs` workgroups with `nk` K-slabs each is split
// `S` ways when it cannot fill the chip (512 resident workgroups): late panels and small batches, where the
// time of a launch is the time of ONE workgroup's K loop.  S is a power of two, every part keeps >= 8 slabs.
#define SF_CHIP_WGS 512
#define SF_SPLIT_MAX 8
static size_t sf_split_region_tiles(void) { return 2 * SF_CHIP_WGS; }  // partial-sum tiles per region
__device__ __forceinline__ size_t sf_split_region_tiles_dev(void) { return 2 * SF_CHIP_WGS; }
static int sf_split_policy(long long wgs, int nk) {
    int S = 1;
    // (a split launch stops at 384 of the 512 slots: two slab groups are in flight and the chain's launches need room --
    // N = 4096, cap 512 / 384 / 256 / 192: B = 16 11.22 / 11.18 / 11.26 / 11.71 ms, 32: 16.06 / 15.78 / 16.09 / 17.28,
    // 64: 27.42 / 27.05 / 26.89 / 28.7)
    while (2 * S <= SF_SPLIT_MAX && wgs * 2 * S <= 384 && nk / (2 * S) >= 8) S *= 2;
    return S;
}
// The scratch of one factorisation of `batch` matrices of order n (the real n, before the frame shift of the fused
// sequences): per matrix a reserved region of SF_LTB_DOUBLES (unused), the panel scratch T and two W^T buffers; then
// the partial-sum tiles: one region for the chain (top) launches, one per slab group.
struct sf_potrf_scratch {
    double* T;  // [batch] x sT
    int64_t sT;
    double* W;  // two buffers of [batch] x sW, one after the other
    int64_t sW;
    double* part;
    int batch;
    size_t doubles;  // the whole scratch: sf_potrf_work_doubles
    double* Wbuf(int i) const { return W + (size_t)i * batch * sW; }
    size_t Wdoubles() const { return 2 * (size_t)batch * sW; }  // both buffers
    // the wide sequence's four most recent inverse tiles W(k): slot k & 3, two 128-row slots to a buffer
    double* Wslot(int k) const { return Wbuf((k >> 1) & 1) + (size_t)(k & 1) * GT * SF_LDT; }
};
static sf_potrf_scratch sf_potrf_scratch_of(double* work, int n, int batch) {
    sf_potrf_scratch w = {};
    const size_t b = (size_t)batch;
    w.sT = (int64_t)(n + SF_NB) * SF_LDT + SF_TSKEW;
    w.sW = (int64_t)SF_NB * SF_LDT + SF_TSKEW;
    w.batch = batch;
    const size_t oT = b * SF_LTB_DOUBLES, oW = oT + b * w.sT, opart = oW + w.Wdoubles() + 64;
    w.doubles = opart + (size_t)(SF_EXEC_GROUPS + 1) * sf_split_region_tiles() * (GT * GT);
    if (work) {
        w.T = work + oT;
        w.W = work + oW;
        w.part = work + opart;
    }
    return w;
}
size_t sf_potrf_work_doubles(int n, int batch) { return sf_potrf_scratch_of(nullptr, n, batch).doubles; }

// The generator fields (matrix-free start) of sf_gemm_args, sf_panel_args and sf_panelw_args, in the frame fp
template <class Args>
static void sf_set_gen(Args& g, const sf_gen_args* gen, int fp) {
    if (!gen) return;
    g.genY = gen->Y - fp;
    g.sY = (int64_t)gen->mpad * gen->ldy;
    g.ldy = gen->ldy;
    g.mpad = gen->mpad;
    g.tilemap = gen->tilemap;
    g.nt128 = gen->nt128;
}
// The fields of sf_panel_args / sf_panelw_args that stay the same over one factorisation (A, rhs and the generator in the
// shifted frame fp)
template <class Args>
static Args sf_panel_frame(double* A, int n, int lda, int64_t stride, double* rhs, int ldr, const sf_gen_args* gen, int fp) {
    Args g = {};
    g.C = A;
    g.sC = stride;
    g.lda = lda;
    g.n = n;
    g.rhs = rhs;
    g.ldr = ldr;
    g.fp = fp;
    sf_set_gen(g, gen, fp);
    return g;
}

// ---- two-stream lookahead ---------------------------------------------------------------------
// The diagonal-block chain is a sequence of small latency-bound launches; it runs on the side stream of
// the caller's sf_exec (owned by the context or by the calling thread) concurrently with the big MFMA
// launches of the caller's stream.
#define SF_TRY(x)          \
    do {                   \
        int rc__ = (x);    \
        if (rc__) return rc__; \
    } while (0)
// fork: the streams `to` (in order) wait for what the caller's stream s holds so far
static int sf_exec_fork(sf_exec* ex, hipStream_t s, std::initializer_list<hipStream_t> to) {
    hipEvent_t e;
    SF_TRY(sf_exec_event(ex, &e));
    SF_HIP(hipEventRecord(e, s));
    for (hipStream_t t : to) SF_HIP(hipStreamWaitEvent(t, e, 0));
    return SF_OK;
}
// join: the caller's stream s continues only after the chain stream c and the launches `also` (NULL: none) are done
static int sf_exec_join(sf_exec* ex, hipStream_t s, hipStream_t c, std::initializer_list<hipEvent_t> also = {}) {
    hipEvent_t e;
    SF_TRY(sf_exec_event(ex, &e));
    SF_HIP(hipEventRecord(e, c));
    SF_HIP(hipStreamWaitEvent(s, e, 0));
    for (hipEvent_t x : also)
        if (x) SF_HIP(hipStreamWaitEvent(s, x, 0));
    return SF_OK;
}
