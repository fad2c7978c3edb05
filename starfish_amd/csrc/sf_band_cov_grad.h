// The covariance gradient of sf_cov_grad.h contracted over the band instead of over the blocks of a dense inverse: with
// C = Bd + Y^T Y, Sigma = Bd^-1 on the band (k_band_selinv, sf_band.hip) and C^-1 = Sigma - Vs Vs^T (Vs = Bd^-1 Y^T L_S^-T),
//     d lnL / d theta = 1/2 sum_{ij on the band} (alpha_i alpha_j - Sigma_ij + (Vs Vs^T)_ij) (dC / d theta)_ij
// because dC / d theta has the support of the kernel itself, which lies inside the band.  A layer of sf_fill.hip: the
// derivative entries, the hyper-parameter read-out, the support test and the reduction frame are those of k_cov_grad.
//
//   k_band_cov_grad  one 4-wave workgroup per (matrix, 64 rows of the lower band).  First the entries
//                    A[i][d] = wgt (alpha_i alpha_j - Sigma_ij + sum_c Vs_ci Vs_cj), j = i - d, c ascending, wgt = 1 on the
//                    diagonal and 2 below it, into LDS (zero where j < 0 or i >= n); then per structured component that
//                    reaches the rows (sf_block_support) the derivative entries on the VALU and its two or three sums,
//                    flushed together in wave order.  Partial sums per (matrix, block row, slot); k_grad_sum adds the block rows.
//                    The entries are dealt to the threads by rows of wp + 1 = 16 (nbr - 1) + 1 >= halfwidth + 1, nbr the
//                    window's block count, those beyond the half-width skipped: every half-width with the same window
//                    gives the same bits (the entries between two such half-widths are zeros of dC / d theta), as the
//                    sweeps do -- a walker keeps its bits whatever group it is evaluated in.
#pragma once
#include "sf_band_shape.h"

struct sf_band_grad_args {
    sf_fill_args f;       // wave, params and the model's layout as the fill gets them (C, Y unused)
    const double* sigma;  // sigma[b * ssigma + i * lds + d] = (Bd^-1)[i][i - d], 0 <= d <= halfwidth
    int64_t ssigma;
    int lds, halfwidth;
    int wp;               // entries per row the threads are dealt: 16 (sfb_nbr(halfwidth) - 1) >= halfwidth, see below
    const double* alpha;  // alpha[b * sstage + i] = (C^-1 r)_i
    const double* vs;     // vs[b * sstage + c * ldv + i] = Vs[i][c], c < m
    int64_t sstage;
    int ldv, m;
    sf_grad_out o;
};

__global__ __launch_bounds__(256) void k_band_cov_grad(const sf_band_grad_args a) {
    extern __shared__ double s_A[];  // [64][wp + 1]
    __shared__ double s_sum[2 + 3 * SF_MAX_LOCAL];
    __shared__ double s_red[12];
    const sf_fill_args& f = a.f;
    const int tid = threadIdx.x, n = f.n, W1 = a.wp + 1;
    int b, I;
    if (!sf_grad_block(a.o, b, I)) return;
    const double* __restrict__ P = f.params + (int64_t)b * f.pstride;
    const double* __restrict__ al = a.alpha + (int64_t)b * a.sstage;
    const double* __restrict__ vs = a.vs + (int64_t)b * a.sstage;
    const double* __restrict__ sg = a.sigma + (int64_t)b * a.ssigma;
    const int R0 = I * 64, rhi = min(R0 + 63, n - 1), clo = max(R0 - a.halfwidth, 0), nent = 64 * W1;
    for (int q = tid; q < a.o.nslots; q += 256) s_sum[q] = 0.0;
    for (int e = tid; e < nent; e += 256) {
        const int ri = e / W1, d = e - ri * W1, i = R0 + ri, j = i - d;
        double v = 0.0;
        if (i < n && j >= 0 && d <= a.halfwidth) {
            double vv = 0.0;
            for (int c = 0; c < a.m; ++c) vv = vv + vs[(int64_t)c * a.ldv + i] * vs[(int64_t)c * a.ldv + j];
            v = (al[i] * al[j] - sg[(int64_t)i * a.lds + d]) + vv;
            if (d > 0) v = 2.0 * v;
        }
        s_A[e] = v;
    }
    sf_global_hyper gh = {0, 1, 0};
    if (f.has_global) gh = sf_load_global(f, P);
    const int gslots = f.has_global ? 2 : 0;
    bool dg;
    unsigned lm;
    sf_block_support(f, P, R0, rhi, clo, rhi, gh.r0, dg, lm);  // (the same in every thread)
    __syncthreads();
    if (dg) {
        double v[3] = {0.0, 0.0, 0.0};
        for (int e = tid; e < nent; e += 256) {
            const int ri = e / W1, d = e - ri * W1, i = R0 + ri, j = i - d;
            if (!(i < n && j >= 0 && d <= a.halfwidth)) continue;
            double k, k_ls;
            sf_matern_grad_elem(f.wave[i], f.wave[j], gh, k, k_ls);
            v[0] = v[0] + s_A[e] * k;
            v[1] = v[1] + s_A[e] * k_ls;
        }
        sf_cov_grad_flush(v, 2, 1.0, s_red, s_sum, tid);
    }
    for (int c = 0; c < f.n_local; ++c) {
        if (!((lm >> c) & 1u)) continue;
        const sf_local_hyper l = sf_load_local(f, P, c);
        double v[3] = {0.0, 0.0, 0.0};
        for (int e = tid; e < nent; e += 256) {
            const int ri = e / W1, d = e - ri * W1, i = R0 + ri, j = i - d;
            if (!(i < n && j >= 0 && d <= a.halfwidth)) continue;
            const double w_r = f.wave[i], w_c = f.wave[j];
            double k, k_mu, k_sig;
            sf_local_grad_elem(sf_local_metric(w_r, l.mu), sf_local_metric_dmu(w_r, l.mu), sf_local_metric(w_c, l.mu),
                               sf_local_metric_dmu(w_c, l.mu), l, k, k_mu, k_sig);
            v[0] = v[0] + s_A[e] * k_mu;
            v[1] = v[1] + s_A[e] * k;
            v[2] = v[2] + s_A[e] * k_sig;
        }
        sf_cov_grad_flush(v, 3, 1.0, s_red, s_sum + gslots + 3 * c, tid);
    }
    __syncthreads();
    double* part = sf_grad_part(a.o, b, I);
    for (int q = tid; q < a.o.nslots; q += 256) part[q] = s_sum[q];
}

// part: sf_cov_grad_work_doubles of scratch; grad[b * grad_stride + slot] in the order of sf_launch_cov_grad; NaN where info[b] != 0
int sf_launch_band_cov_grad(const sf_fill_args& f, int batch, const double* sigma, int lds, int64_t ssigma, int halfwidth,
                            const double* alpha, const double* vs, int ldv, int64_t sstage, int m, const int* info, double* part,
                            double* grad, int grad_stride, hipStream_t s) {
    SF_CHECK(sf_check_n_local(f));
    sf_band_grad_args a;
    a.f = f;
    a.sigma = sigma, a.ssigma = ssigma, a.lds = lds, a.halfwidth = halfwidth, a.wp = BB * (sfb_nbr(halfwidth) - 1);
    a.alpha = alpha, a.vs = vs, a.sstage = sstage, a.ldv = ldv, a.m = m;
    static const int wmax = sf_band_max_halfwidth(1);  // the widest band any window takes
    a.o = sf_grad_out{info, part, (f.n + 63) / 64, sf_cov_grad_slots(f.has_global, f.n_local), batch, grad, grad_stride};
    if (f.n <= 0 || !f.monotonic || halfwidth < 0 || halfwidth > wmax || lds < halfwidth + 1 || ldv < f.n || m < 1 ||
        a.o.nslots < 1 || grad_stride < a.o.nslots || batch < 1 || batch > 65535) {
        sf_set_error("band cov grad: n, a sorted grid, half-width in 0 .. %d, lds > half-width, ldv >= n, a structured kernel, "
                     "grad_stride >= slots, batch in 1 .. 65535", wmax);
        return SF_EINVAL;
    }
    const size_t shm = sizeof(double) * 64 * (size_t)(a.wp + 1);
    static sf_dev_once attr_once;
    SF_CHECK(sf_lds_limit_once(&attr_once, (int)(sizeof(double) * 64 * (BB * (sfb_nbr(wmax) - 1) + 1)), {(const void*)k_band_cov_grad}));
    const long long grid = (long long)batch * a.o.nbr;
    SF_CHECK(sf_check_fill_grid(grid));
    hipLaunchKernelGGL(k_band_cov_grad, dim3((unsigned)grid), dim3(256), shm, s, a);
    SF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_grad_sum, dim3((a.o.nslots + 63) / 64, batch), dim3(64), 0, s, a.o);
    SF_LAUNCH_CHECK();
    return SF_OK;
}
