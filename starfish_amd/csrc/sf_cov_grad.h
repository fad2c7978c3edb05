// The likelihood's gradient in the covariance hyper-parameters: the contraction of sf_grad_frame.h with
// theta = log_amp, log_ls of the global kernel and mu, log_amp, log_sigma of every local kernel.  dC / d theta has the
// support of the kernel itself, so only the 64 x 64 blocks of C^-1 that sf_block_support flags are formed.  A layer of
// sf_fill.hip: the support test and the hyper-parameter read-out are the fill's; the derivative formulas are this layer's own
// (they need not share bits with the fill).
//
//   k_cov_grad       the frame's block-row kernel.  It walks J = 0 .. I in order; the support of every pair is asked once
//                    (one thread per pair, flags in LDS); per supported pair the tile and per structured component that
//                    reaches the pair the derivative entries on the VALU (an exp, a cos and a sin per entry), one component
//                    at a time, its two or three sums flushed together.
#pragma once

#define SF_GRAD_SB 256  // pairs of a block row whose support flags are held at a time (n <= 16384: all of them)

// ---- derivative entries.  kernels.py:27-40 with u = r / ls, t = 1/2 + 1/2 cos(pi u / 6), g = (1 + sqrt(3) u) e^(-sqrt(3) u):
// K = A t g,  dK / d log_amp = K,  dK / d log_ls = -u A (t' g + t g'),  t' = -(pi / 12) sin(pi u / 6),  g' = -3 u e^(-sqrt(3) u)
__device__ __forceinline__ void sf_matern_grad_elem(double w_row, double w_col, const sf_global_hyper& h, double& k, double& k_ls) {
    k = 0.0, k_ls = 0.0;
    const double r = SF_C_KMS / 2 * fabs((w_col - w_row) / (w_col + w_row));
    if (!(r <= h.r0)) return;
    const double s3 = 1.7320508075688772;
    const double u = r / h.ls, ph = M_PI * u / 6;
    const double t = 0.5 + 0.5 * cos(ph), tp = -(M_PI / 12) * sin(ph);
    const double e = exp(-s3 * u), g = (1 + s3 * u) * e, gp = -3 * u * e;
    k = h.amp * t * g;
    k_ls = -u * h.amp * (tp * g + t * gp);
}
// kernels.py:69-80 with d(w) = c / mu |w - mu|, d' = dd / dmu = -c sign(w - mu) w / mu^2, v = r_tap / sigma,
// e = exp(-r2 / (2 sigma^2)), t = 1/2 + 1/2 cos(pi v / 4), s = 1/2 sin(pi v / 4); r_tap' = d' of the larger metric (the
// column's on a tie, as the fill's fmax(d_col, d_row)):
// K = A t e,  dK / d log_sigma = A e (s pi v / 4 + t r2 / sigma^2),
// dK / d mu = A e (-s pi / (4 sigma) r_tap' - t (d_col d_col' + d_row d_row') / sigma^2)
__device__ __forceinline__ double sf_local_metric_dmu(double w, double mu) {
    const double sg = w > mu ? 1.0 : (w < mu ? -1.0 : 0.0);
    return -SF_C_KMS * sg * w / (mu * mu);
}
__device__ __forceinline__ void sf_local_grad_elem(double d_row, double dp_row, double d_col, double dp_col, const sf_local_hyper& l,
                                                   double& k, double& k_mu, double& k_sig) {
    k = 0.0, k_mu = 0.0, k_sig = 0.0;
    const bool col = d_col >= d_row;
    const double r_tap = col ? d_col : d_row, r_tap_p = col ? dp_col : dp_row;
    if (!(r_tap <= 4 * l.sig)) return;
    const double is2 = 1.0 / (l.sig * l.sig);
    const double r2 = d_col * d_col + d_row * d_row;
    const double v = r_tap / l.sig, ph = M_PI * v / 4;
    const double t = 0.5 + 0.5 * cos(ph), sn = 0.5 * sin(ph);
    const double ae = l.amp * exp(-0.5 * r2 * is2);
    k = ae * t;
    k_sig = ae * (sn * ph + t * r2 * is2);
    k_mu = ae * (-sn * (M_PI / 4) / l.sig * r_tap_p - t * (d_col * dp_col + d_row * dp_row) * is2);
}

struct sf_grad_args {
    sf_fill_args f;       // wave, params and the model's layout as the fill gets them (C: the factored matrices, X^T above)
    const double* winv;   // [batch][npad / 64][64][64]
    const double* alpha;  // [batch][lda_alpha]: C^-1 r, n data rows
    int ld_alpha;
    sf_grad_out o;
};

// a component's sums over the pair (the third is zero where it has two), added times wgt to its running sums
__device__ __forceinline__ void sf_cov_grad_flush(const double (&v)[3], int nv, double wgt, double* red, double* sums, int tid) {
#pragma unroll
    for (int q = 0; q < 3; ++q) sf_grad_put(v[q], red + (tid >> 6) * 3 + q, tid & 63);
    sf_grad_flush(nv, wgt, red, 3, sums, tid);
}

__global__ __launch_bounds__(256) void k_cov_grad(const sf_grad_args a) {
    __shared__ unsigned s_lmask[SF_GRAD_SB];
    __shared__ unsigned char s_glob[SF_GRAD_SB];
    __shared__ double s_sum[2 + 3 * SF_MAX_LOCAL];
    __shared__ double s_red[12];
    const sf_fill_args& f = a.f;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, lq = lane >> 4;
    const int n = f.n;
    int b, I;
    if (!sf_grad_block(a.o, b, I)) return;
    const double* __restrict__ P = f.params + (int64_t)b * f.pstride;
    const double* __restrict__ al = a.alpha + (int64_t)b * a.ld_alpha;
    const sf_cinv_src src = sf_cinv_source(f.C, f.npad, f.lda, f.stride, a.winv, b);
    sf_global_hyper gh = {0, 1, 0};
    if (f.has_global) gh = sf_load_global(f, P);
    const int gslots = f.has_global ? 2 : 0;
    for (int q = tid; q < a.o.nslots; q += 256) s_sum[q] = 0.0;
    const int R0 = I * 64, rhi = min(R0 + 63, n - 1);
    double w_r[4], a_r[4];  // wavelength and alpha of this thread's rows
    bool ok_r[4];
    sf_grad_rows(al, R0, n, w, lq, a_r, ok_r);
#pragma unroll
    for (int r = 0; r < 4; ++r) w_r[r] = ok_r[r] ? f.wave[R0 + 16 * w + lq + 4 * r] : 1.0;
    for (int sb0 = 0; sb0 <= I; sb0 += SF_GRAD_SB) {
        const int nsb = min(SF_GRAD_SB, I + 1 - sb0);
        __syncthreads();  // the flags of the last chunk are read; s_sum is zeroed
        if (tid < nsb) {
            const int clo = (sb0 + tid) * 64;
            bool dg;
            unsigned lm;
            sf_block_support(f, P, R0, rhi, clo, min(clo + 63, n - 1), gh.r0, dg, lm);
            s_glob[tid] = dg ? 1 : 0;
            s_lmask[tid] = lm;
        }
        __syncthreads();
        for (int jj = 0; jj < nsb; ++jj) {
            const bool dg = s_glob[jj] != 0;
            const unsigned lm = s_lmask[jj];
            if (!dg && !lm) continue;  // (the same in every thread)
            const int J = sb0 + jj, C0 = J * 64;
            const double wgt = sf_grad_weight(I, J);
            sf_d4 A[4];
            double w_c[4];  // wavelength of this thread's columns 16 t + l15 of block J
            bool ok_c[4];
            sf_grad_tile(src, al, n, I, J, w, l15, lq, a_r, ok_r, A, ok_c);
#pragma unroll
            for (int t = 0; t < 4; ++t) w_c[t] = ok_c[t] ? f.wave[C0 + 16 * t + l15] : 1.0;
            if (dg) {
                double v[3] = {0.0, 0.0, 0.0};
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if (!(ok_r[r] && ok_c[t])) continue;
                        double k, k_ls;
                        sf_matern_grad_elem(w_r[r], w_c[t], gh, k, k_ls);
                        v[0] = v[0] + A[t][r] * k;
                        v[1] = v[1] + A[t][r] * k_ls;
                    }
                sf_cov_grad_flush(v, 2, wgt, s_red, s_sum, tid);
            }
            for (int c = 0; c < f.n_local; ++c) {
                if (!((lm >> c) & 1u)) continue;
                const sf_local_hyper l = sf_load_local(f, P, c);
                double d_r[4], dp_r[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    d_r[r] = sf_local_metric(w_r[r], l.mu);
                    dp_r[r] = sf_local_metric_dmu(w_r[r], l.mu);
                }
                double v[3] = {0.0, 0.0, 0.0};
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const double d_c = sf_local_metric(w_c[t], l.mu), dp_c = sf_local_metric_dmu(w_c[t], l.mu);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if (!(ok_r[r] && ok_c[t])) continue;
                        double k, k_mu, k_sig;
                        sf_local_grad_elem(d_r[r], dp_r[r], d_c, dp_c, l, k, k_mu, k_sig);
                        v[0] = v[0] + A[t][r] * k_mu;
                        v[1] = v[1] + A[t][r] * k;
                        v[2] = v[2] + A[t][r] * k_sig;
                    }
                }
                sf_cov_grad_flush(v, 3, wgt, s_red, s_sum + gslots + 3 * c, tid);
            }
        }
    }
    __syncthreads();
    double* part = sf_grad_part(a.o, b, I);
    for (int q = tid; q < a.o.nslots; q += 256) part[q] = s_sum[q];
}

size_t sf_cov_grad_work_doubles(int n, int has_global, int n_local, int batch) {
    if (n <= 0 || batch <= 0) return 0;
    return sf_grad_part_doubles(n, sf_cov_grad_slots(has_global, n_local), batch);
}
int sf_launch_cov_grad(const sf_fill_args& f, int batch, const double* winv, const double* alpha, int ld_alpha, const int* info,
                       double* part, double* grad, int grad_stride, hipStream_t s) {
    SF_CHECK(sf_check_n_local(f));
    sf_grad_args a;
    a.f = f;
    a.winv = winv, a.alpha = alpha, a.ld_alpha = ld_alpha;
    a.o = sf_grad_out{info, part, (f.n + 63) / 64, sf_cov_grad_slots(f.has_global, f.n_local), batch, grad, grad_stride};
    if (f.n <= 0 || f.npad % SF_LEAF != 0 || f.npad < f.n || a.o.nslots < 1 || grad_stride < a.o.nslots || ld_alpha < f.n || batch < 1 ||
        batch > 65535) {
        sf_set_error("cov grad: n, npad a multiple of %d, a structured kernel, grad_stride >= slots, ld_alpha >= n, batch in 1 .. 65535",
                     SF_LEAF);
        return SF_EINVAL;
    }
    return sf_launch_grad(k_cov_grad, a, a.o, s);
}
