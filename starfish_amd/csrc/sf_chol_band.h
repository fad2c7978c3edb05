// Bordered band matrices on the fused panel kernel: the border / finish kernels and the driver sf_launch_potrf_band.
// Used by the band solver in sf_banded.cpp for half-widths beyond the LDS window of k_band_forms.
#pragma once
#include "sf_chol_host.h"
#include "sf_chol_panel.h"
#include "sf_chol_seq.h"

// ---------------------------------------------------------------------------------------------
// Bordered band matrices on the fused panel kernel (the structure-exploiting solver for half-widths beyond the
// LDS window of k_band_forms):
//
//        [ Bd   .  ]      Bd: nband x nband, zero further than `halfwidth` from the diagonal (128 x 128 tiles of a
//    A = [         ]          dense-strided array; only the tiles that meet the band are ever touched)
//        [ R    G  ]      R:  the 1 + m right-hand sides as 64 extra ROWS,  G = 0
//
// Left-looking panels exactly as in sf_launch_potrf_v2, but rest(k) covers only the slabs that meet the band plus the
// border slab, and every slab's K loop starts at its first non-zero column: O(n W^2) flops on kernels that run at
// the dense path's rate, spread over the whole chip (round 1's in-place sweep kept one matrix on one CU and streamed
// its operands from L2: 7.5 / 10.3 / 30.1 ms at W = 241 / 361 / 724 against 5.0 / 6.0 / 11.3 here).  The border rows come out as Z = R L^-T, their diagonal tile as -Z Z^T: the Gram matrix the
// Woodbury step needs; L_band's diagonal gives logdet(Bd).  The diagonal tile of the border is never factorised.
// border rows: the right-hand sides (sf_band_rhs), everything else (and the border's own diagonal tile) zero
__global__ __launch_bounds__(256) void k_band_border_rows(sf_band_rhs rhs, int n, int nband, double* __restrict__ A, int64_t sA, int lda) {
    const int b = blockIdx.z, r = blockIdx.y, col = blockIdx.x * 256 + threadIdx.x;
    if (col >= nband + 64) return;
    const double v = r < rhs.nrhs && col < n ? rhs.of(b).row(r)[col] : 0.0;
    A[(int64_t)b * sA + (int64_t)(nband + r) * lda + col] = v;
}
__global__ __launch_bounds__(256) void k_band_tiles_finish(const double* __restrict__ A, int64_t sA, int lda, int nband, int nrhs,
                                                           double* __restrict__ logdet, double* __restrict__ gram) {
    __shared__ double red[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const double* Ab = A + (int64_t)b * sA;
    double acc = 0.0;
    for (int i = tid; i < nband; i += 256) acc += log(Ab[(int64_t)i * lda + i]);
    red[tid] = acc;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) red[tid] += red[tid + st];
        __syncthreads();
    }
    if (tid == 0) logdet[b] = 2.0 * red[0];
    for (int e = tid; e < nrhs * nrhs; e += 256) {
        const int r = e / nrhs, c = e - r * nrhs;
        gram[(int64_t)b * nrhs * nrhs + e] = -Ab[(int64_t)(nband + max(r, c)) * lda + nband + min(r, c)];
    }
}

int sf_band_tiles_lda(int nband) { return nband + 64 + 16; }
int sf_band_tiles_wt(int halfwidth) { return (halfwidth + GT - 1) / GT; }
size_t sf_band_tiles_doubles(int nband, int batch) {  // the dense-strided array + the factorisation's scratch
    return (size_t)batch * (nband + 64) * sf_band_tiles_lda(nband) + sf_potrf_work_doubles(nband + 64, batch) + 64;
}

// The lower 128 x 128 tiles that meet the band are in place at the start of `tiles` (k_band_fill's tile mode: row
// stride sf_band_tiles_lda(nband), nband + 64 rows per matrix, zeros where the band ends inside a tile, identity
// padding from n to nband = n rounded up to 64); `tiles` holds sf_band_tiles_doubles(nband, batch) doubles.  c.r: the
// right-hand sides (as for sf_launch_band_forms; c.band is not read).  Outputs logdet(Bd) and the nrhs x nrhs
// Gram matrix of the solved right-hand sides; info[b] (cleared by the caller) gets the first non-positive pivot.
int sf_launch_potrf_band(const sf_band_call& c, int nband, double* tiles, hipStream_t s) {
    const int n = c.n, halfwidth = c.halfwidth, batch = c.batch, nrhs = c.r.nrhs;
    int* const info = c.info;
    if (nband % SF_LEAF != 0 || nband < n || batch <= 0 || nrhs < 1 || nrhs > 64 || halfwidth < 0 || !tiles) {
        sf_set_error("potrf_band: bad arguments (n=%d nband=%d halfwidth=%d nrhs=%d)", n, nband, halfwidth, nrhs);
        return SF_EINVAL;
    }
    const int next = nband + 64, lda = sf_band_tiles_lda(nband);
    const int64_t sA = (int64_t)next * lda;
    double* A = tiles;
    double* work = tiles + (size_t)batch * sA;
    const int nt = (nband + GT - 1) / GT;
    const int wt = sf_band_tiles_wt(halfwidth);

    hipLaunchKernelGGL(k_band_border_rows, dim3((next + 255) / 256, 64, batch), dim3(256), 0, s, c.r, n, nband, A, sA, lda);
    SF_LAUNCH_CHECK();

    const sf_potrf_scratch ws = sf_potrf_scratch_of(work, next, batch);  // (one W buffer is used)
    // (info is NOT cleared here: the band fill may have flagged a half-width that is too small; a non-zero entry stays)
    // One stream, two launches per panel: the launches are short (a few slabs, K <= halfwidth + 128), so the
    // lookahead of the dense sequence has nothing to hide behind -- measured with the chain on a side stream:
    // 13.4 ms against 9.4 at W = 361 (cross-stream waits cost more than the kernels they overlap).
    auto launch_panel = [&](int k0, int pw, int row0, int nslab, bool border) -> int {
        sf_panel_args g = {};
        g.C = A;
        g.sC = sA;
        g.lda = lda;
        g.n = next;
        g.k0 = k0;
        g.pw = pw;
        g.row0 = row0;
        g.nslab = nslab + (border ? 1 : 0);
        g.slab_step = 1;
        g.Wt = ws.W;
        g.sW = ws.sW;
        g.kband = halfwidth > 0 ? halfwidth : 1;
        g.nband = nband;
        g.xrow0 = border ? nband : 0;
        if (nslab > 0) sf_park(g, ws);  // the first slab is the next diagonal tile: its update is parked in the scratch for D(k+1)
        const long long nblk = (long long)g.nslab * batch;
        if (nblk <= 0) return SF_OK;
        void* tok;
        sf_prof_gemm_begin(s, 2.0 * (double)min(k0, halfwidth + GT) * GT * pw * (double)nblk, &tok);
        hipLaunchKernelGGL((k_chol_panel<false, 0>), dim3((unsigned)nblk), dim3(512), 0, s, g);
        sf_prof_gemm_end(tok);
        SF_LAUNCH_CHECK();
        return SF_OK;
    };
    SF_TRY(launch_panel(0, 0, 0, 1, false));  // diagonal tile 0 goes to the scratch unchanged
    for (int k = 0; k < nt; ++k) {
        const int k0 = k * GT;
        const int pw = (nband - k0 < GT) ? nband - k0 : GT;
        SF_TRY(sf_diag_step(ws, A, lda, sA, nullptr, 0, info, nband, k, ws.W, 0, s));
        // the slabs k+1 .. k+wt that meet the band, and the border
        const int last = (k + wt < nt - 1) ? k + wt : nt - 1;
        SF_TRY(launch_panel(k0, pw, (k + 1) * GT, last - k, true));
    }
    hipLaunchKernelGGL(k_band_tiles_finish, dim3(batch), dim3(256), 0, s, A, sA, lda, nband, nrhs, c.logdet, c.gram);
    SF_LAUNCH_CHECK();
    return SF_OK;
}
