// The Fisher information of the mean-flux parameters for all orders of a multi-order call (sf_fisher_banded_multi_batch_md,
// sf_multi_fisher_reduce).  A layer of sf_transform.hip ("Fisher information of an echelle model"); the sweep's rows
// and the Gram step are sf_fisher.h's, launched over the units of every order at once in ONE frame of 1 + m + pmax rows:
//   spread     k_fisher_spread: k_fisher_band stays what it was -- its leading dimension is its column count, here the frame's
//              pmax -- and leaves compact pmax x pmax blocks; this kernel copies them into the caller's (ld, stride) layout.  An
//              order with fewer columns carries zero rows behind its own: exact zeros in the Gram matrix and in U, so its
//              p_i x p_i block is what it would be alone and the rest of the pmax x pmax block is 0 (or NaN with the unit).
//   reduce     k_multi_fisher_reduce: the sum of the unit matrices over the orders, per (walker, pair of labels a >= b), through
//              the column map of sf_multi_grad_reduce: a two-pointer merge of the two labels' source lists picks the segments
//              that appear in both, ascending, s = f_0; s = s + f_1; ...; no common segment: 0.0.  The lower triangle is
//              mirrored, so F_ab and F_ba are the same bits.  Plain adds, no atomics.
#pragma once
#include "sf_fisher.h"

// fisher[u * fstride + a * ld + b] = comp[u][a][b], a, b < p
__global__ __launch_bounds__(64) void k_fisher_spread(const double* __restrict__ comp, int p, double* __restrict__ fisher, int ld,
                                                      int64_t fstride) {
    const double* __restrict__ c = comp + (int64_t)blockIdx.x * p * p;
    double* __restrict__ F = fisher + (int64_t)blockIdx.x * fstride;
    for (int e = threadIdx.x; e < p * p; e += 64) F[(e / p) * ld + (e % p)] = c[e];
}
int sf_launch_fisher_spread(const double* comp, int p, int batch, double* fisher, int ld, int64_t fstride, hipStream_t s) {
    if (!comp || !fisher || p < 1 || p > SF_MEAN_GRAD_MAX_SLOTS || batch <= 0 || ld < p || fstride < (int64_t)ld * (p - 1) + p) {
        sf_set_error("fisher spread: nslots=%d / ld=%d / stride not supported", p, ld);
        return SF_EINVAL;
    }
    hipLaunchKernelGGL(k_fisher_spread, dim3(batch), dim3(64), 0, s, comp, p, fisher, ld, fstride);
    SF_LAUNCH_CHECK();
    return SF_OK;
}

// One thread per (pair, walker); the pair index runs fastest: neighbouring threads write neighbouring entries of a row of
// the lower triangle and read the same few entries of the column map (the walkers' unit matrices lie fisher_stride apart
// whichever index runs fastest).  Pair npair is the walker's lnl and status, by k_multi_grad_reduce's rule.
__global__ __launch_bounds__(256) void k_multi_fisher_reduce(const sf_multi_fisher_reduce_args a) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, npair = (int64_t)a.ncols * (a.ncols + 1) / 2;
    const int w = blockIdx.y;
    if (e > npair) return;
    int code = 0;
    for (int i = 0; i < a.nseg && code == 0; ++i) code = a.unit_info[(int64_t)i * a.W + w];
    if (e == npair) {
        double s = a.unit_lnl[w];
        for (int i = 1; i < a.nseg; ++i) s = s + a.unit_lnl[(int64_t)i * a.W + w];
        a.lnl[w] = code != 0 ? -__builtin_inf() : s;
        a.info[w] = code;
        return;
    }
    int r = (int)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);  // row of the lower triangle: r (r + 1) / 2 <= e
    while ((int64_t)(r + 1) * (r + 2) / 2 <= e) ++r;
    while ((int64_t)r * (r + 1) / 2 > e) --r;
    const int c = (int)(e - (int64_t)r * (r + 1) / 2);
    double s = 0.0;
    if (code != 0) {
        s = __builtin_nan("");
    } else {
        int qa = a.col_ptr[r], qb = a.col_ptr[c];
        const int ea = a.col_ptr[r + 1], eb = a.col_ptr[c + 1];
        bool first = true;
        while (qa < ea && qb < eb) {
            const int ia = a.col_src[2 * qa], ib = a.col_src[2 * qb];
            if (ia < ib) {
                ++qa;
            } else if (ib < ia) {
                ++qb;
            } else {
                const int sa = a.col_src[2 * qa + 1], sb = a.col_src[2 * qb + 1];
                double f = __builtin_nan("");
                if (ia >= 0 && ia < a.nseg && sa >= 0 && sa < a.fisher_ld && sb >= 0 && sb < a.fisher_ld)
                    f = a.unit_fisher[((int64_t)ia * a.W + w) * a.fisher_stride + (int64_t)sa * a.fisher_ld + sb];
                s = first ? f : s + f;
                first = false;
                ++qa, ++qb;
            }
        }
    }
    double* __restrict__ F = a.fisher + (int64_t)w * a.out_stride;
    F[(int64_t)r * a.ncols + c] = s;
    F[(int64_t)c * a.ncols + r] = s;
}
int sf_launch_multi_fisher_reduce(const sf_multi_fisher_reduce_args& a, hipStream_t s) {
    if (a.nseg < 1 || a.W < 1 || a.W > 65535 || a.ncols < 0 || a.ncols > 32768 || a.fisher_ld < 1 ||
        a.fisher_stride < (int64_t)a.fisher_ld * a.fisher_ld || a.out_stride < (int64_t)a.ncols * a.ncols) {
        sf_set_error("sf_multi_fisher_reduce: nseg >= 1, W in 1 .. 65535, ncols in 0 .. 32768, fisher_ld >= 1, fisher_stride >= "
                     "fisher_ld^2 and out_stride >= ncols^2");
        return SF_EINVAL;
    }
    const int64_t npair = (int64_t)a.ncols * (a.ncols + 1) / 2;
    hipLaunchKernelGGL(k_multi_fisher_reduce, dim3((unsigned)((npair + 1 + 255) / 256), a.W), dim3(256), 0, s, a);
    SF_LAUNCH_CHECK();
    return SF_OK;
}
