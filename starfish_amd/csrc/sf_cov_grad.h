// The likelihood's gradient in the covariance hyper-parameters (Rasmussen & Williams, Gaussian Processes for Machine
// Learning, eq. 5.9):
//     d lnL / d theta = 1/2 sum_ij (alpha_i alpha_j - (C^-1)_ij) (dC / d theta)_ij,   alpha = C^-1 r,  C^-1 = X^T X,  X = L^-1
// for theta = log_amp, log_ls of the global kernel and mu, log_amp, log_sigma of every local kernel.  dC / d theta has the
// support of the kernel itself, so only the 64 x 64 blocks of C^-1 that sf_block_support flags are formed.  X is what
// sf_launch_chol_inverse_diag leaves: X_KJ (K > J) transposed in the strict upper triangle (row 64 J + c, columns 64 K ..),
// X_JJ transposed in winv[J], zero above its diagonal.  A layer of sf_fill.hip: the support test and the hyper-parameter
// read-out are the fill's; the derivative formulas are this layer's own (they need not share bits with the fill).
//
//   sf_cinv_tile     G_IJ = sum_{K >= I} X_KI^T X_KJ for J <= I on v_mfma_f64_16x16x4_f64: both operands are k-contiguous
//                    (sf_inv_sweep).  Four waves; wave w holds rows 16 w .. 16 w + 15 of block I against the 64 columns of
//                    block J in four accumulators, register r of acc[t] = (row 16 w + lq + 4 r, column 16 t + l15).
//   k_cinv_blocks    one workgroup per (matrix, listed pair): the tile, stored (sf_potri_blocks_batch).
//   k_cov_grad       one workgroup per (walker, block row I), short I first (their K sums are the long ones).  It walks
//                    J = 0 .. I in order; the support of every pair is asked once (one thread per pair, flags in LDS); per
//                    supported pair the tile, A_ij = alpha_i alpha_j - G_ij for i, j < n, and per structured component that
//                    reaches the pair the derivative entries on the VALU (an exp, a cos and a sin per entry), one component
//                    at a time.  A component's sums over the pair meet in LDS (lanes by xor shuffles, then the four waves in
//                    order) and thread 0 adds them, weighted 2 off the diagonal pair and 1 on it, to the running sum of the
//                    slot.  Partial sums per (walker, block row, slot) go to the workspace.
//   k_cov_grad_sum   one thread per (walker, slot): the block rows in ascending order, times 1/2; NaN where info != 0.
// No atomics, no workgroup waits for another, every sum in a fixed order (a repeated call gives the same bits); nothing of
// the lower triangle is written; rows and columns >= n are not read as data (their alpha and entries are masked) and
// nothing is written for them.
#pragma once

#define SF_GRAD_SB 256  // pairs of a block row whose support flags are held at a time (n <= 16384: all of them)

struct sf_cinv_src {
    const double* Mx;    // the matrix: L below, X^T above
    const double* Wb;    // winv of the matrix: [nb][64][64]
    int n, lda;          // n: order, a multiple of 64
    bool al_l, al_w;     // rows of Mx / winv 16-byte aligned
};
__device__ __forceinline__ sf_cinv_src sf_cinv_source(const double* L, int n, int lda, int64_t stride, const double* winv, int b) {
    sf_cinv_src s;
    s.Mx = L + (int64_t)b * stride;
    s.Wb = winv + (int64_t)b * (n / SF_LEAF) * (SF_LEAF * SF_LEAF);
    s.n = n, s.lda = lda;
    s.al_l = (((uintptr_t)s.Mx & 15) | (lda & 1)) == 0;
    s.al_w = ((uintptr_t)winv & 15) == 0;
    return s;
}
// 0 <= J <= I < n / 64 (the caller's check)
__device__ __forceinline__ void sf_cinv_tile(const sf_cinv_src& s, int I, int J, int w, int l15, int lq, sf_d4 (&acc)[4]) {
    const int r0 = I * SF_LEAF, c0 = J * SF_LEAF;
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = sf_d4{0.0, 0.0, 0.0, 0.0};
    // column i of X indexed by the absolute k: in winv (K = block of i) and in the upper triangle (K beyond it)
    const double* WI = s.Wb + (int64_t)I * (SF_LEAF * SF_LEAF);
    const double* aw = WI + (16 * w + l15) * SF_LEAF - r0;
    const double* au = s.Mx + (int64_t)(r0 + 16 * w + l15) * s.lda;
    const double *xw[4], *xu[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        xw[t] = WI + (16 * t + l15) * SF_LEAF - r0;  // (used where J == I)
        xu[t] = s.Mx + (int64_t)(c0 + 16 * t + l15) * s.lda;
    }
    if (J == I)
        sf_inv_sweep(aw, s.al_w, xw, s.al_w, r0, r0 + SF_LEAF, lq, acc);
    else
        sf_inv_sweep(aw, s.al_w, xu, s.al_l, r0, r0 + SF_LEAF, lq, acc);
    sf_inv_sweep(au, s.al_l, xu, s.al_l, r0 + SF_LEAF, s.n, lq, acc);
}

struct sf_cinv_blocks_args {
    const double* L;
    int n, lda;
    int64_t stride;
    const double* winv;
    const int* pairs;  // [npairs][2]: I, J
    int npairs;
    double* out;       // [batch][npairs][64][64]
};
__global__ __launch_bounds__(256) void k_cinv_blocks(const sf_cinv_blocks_args a) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, lq = lane >> 4;
    const int p = blockIdx.x % a.npairs, b = blockIdx.x / a.npairs;
    const int I = a.pairs[2 * p], J = a.pairs[2 * p + 1];
    double* out = a.out + ((int64_t)b * a.npairs + p) * (SF_LEAF * SF_LEAF);
    sf_d4 acc[4];
    if (J < 0 || J > I || I >= a.n / SF_LEAF) {  // a pair outside the matrix: nothing is read
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = sf_d4{__builtin_nan(""), __builtin_nan(""), __builtin_nan(""), __builtin_nan("")};
    } else {
        sf_cinv_tile(sf_cinv_source(a.L, a.n, a.lda, a.stride, a.winv, b), I, J, w, l15, lq, acc);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) out[(16 * w + lq + 4 * r) * SF_LEAF + 16 * t + l15] = acc[t][r];
}
int sf_launch_cinv_blocks(const double* L, int n, int lda, int64_t stride, int batch, const double* winv, const int* pairs,
                          int npairs, double* out, hipStream_t s) {
    sf_cinv_blocks_args a;
    a.L = L, a.n = n, a.lda = lda, a.stride = stride, a.winv = winv, a.pairs = pairs, a.npairs = npairs, a.out = out;
    const long long grid = (long long)batch * npairs;
    SF_CHECK(sf_check_fill_grid(grid));
    hipLaunchKernelGGL(k_cinv_blocks, dim3((unsigned)grid), dim3(256), 0, s, a);
    SF_LAUNCH_CHECK();
    return SF_OK;
}

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
    const int* info;      // [batch]: != 0 -> NaN rows, nothing is read
    double* part;         // [batch][nbr][nslots]
    int nbr, nslots, batch;
    double* grad;         // [batch][grad_stride]
    int grad_stride;
};

// the sums of up to three values over the workgroup, added (times wgt) to the running sums sums[0 .. nv) by thread 0
__device__ __forceinline__ void sf_grad_reduce(double (&v)[3], int nv, double wgt, double* red, double* sums, int tid) {
    const int lane = tid & 63, w = tid >> 6;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        v[q] = sf_wave_sum(v[q]);
        if (lane == 0) red[w * 3 + q] = v[q];
    }
    __syncthreads();
    if (tid == 0)
        for (int q = 0; q < nv; ++q) sums[q] = sums[q] + wgt * (((red[q] + red[3 + q]) + red[6 + q]) + red[9 + q]);
    __syncthreads();
}

__global__ __launch_bounds__(256) void k_cov_grad(const sf_grad_args a) {
    __shared__ unsigned s_lmask[SF_GRAD_SB];
    __shared__ unsigned char s_glob[SF_GRAD_SB];
    __shared__ double s_sum[2 + 3 * SF_MAX_LOCAL];
    __shared__ double s_red[12];
    const sf_fill_args& f = a.f;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, lq = lane >> 4;
    const int b = blockIdx.x % a.batch, I = blockIdx.x / a.batch, n = f.n;
    if (a.info[b] != 0) return;  // (k_cov_grad_sum writes NaN and does not read the partial sums)
    const double* __restrict__ P = f.params + (int64_t)b * f.pstride;
    const double* __restrict__ al = a.alpha + (int64_t)b * a.ld_alpha;
    const sf_cinv_src src = sf_cinv_source(f.C, f.npad, f.lda, f.stride, a.winv, b);
    sf_global_hyper gh = {0, 1, 0};
    if (f.has_global) gh = sf_load_global(f, P);
    const int gslots = f.has_global ? 2 : 0;
    for (int q = tid; q < a.nslots; q += 256) s_sum[q] = 0.0;
    const int R0 = I * 64, rhi = min(R0 + 63, n - 1);
    // this thread's rows 16 w + lq + 4 r of block I: wavelength, alpha, masked beyond n
    double w_r[4], a_r[4];
    bool ok_r[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = R0 + 16 * w + lq + 4 * r;
        ok_r[r] = i < n;
        w_r[r] = ok_r[r] ? f.wave[i] : 1.0;
        a_r[r] = ok_r[r] ? al[i] : 0.0;
    }
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
            const double wgt = J < I ? 2.0 : 1.0;
            sf_d4 A[4];
            sf_cinv_tile(src, I, J, w, l15, lq, A);
            // this thread's columns 16 t + l15 of block J; A_ij = alpha_i alpha_j - G_ij, zero beyond n
            double w_c[4];
            bool ok_c[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int j = C0 + 16 * t + l15;
                ok_c[t] = j < n;
                w_c[t] = ok_c[t] ? f.wave[j] : 1.0;
                const double a_c = ok_c[t] ? al[j] : 0.0;
#pragma unroll
                for (int r = 0; r < 4; ++r) A[t][r] = ok_r[r] && ok_c[t] ? a_r[r] * a_c - A[t][r] : 0.0;
            }
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
                sf_grad_reduce(v, 2, wgt, s_red, s_sum, tid);
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
                sf_grad_reduce(v, 3, wgt, s_red, s_sum + gslots + 3 * c, tid);
            }
        }
    }
    __syncthreads();
    double* part = a.part + ((int64_t)b * a.nbr + I) * a.nslots;
    for (int q = tid; q < a.nslots; q += 256) part[q] = s_sum[q];
}

__global__ void k_cov_grad_sum(const sf_grad_args a) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (q >= a.nslots) return;
    double s = 0.0;
    if (a.info[b] != 0) {
        s = __builtin_nan("");
    } else {
        for (int I = 0; I < a.nbr; ++I) s = s + a.part[((int64_t)b * a.nbr + I) * a.nslots + q];
        s = 0.5 * s;
    }
    a.grad[(int64_t)b * a.grad_stride + q] = s;
}

size_t sf_cov_grad_work_doubles(int n, int has_global, int n_local, int batch) {
    if (n <= 0 || batch <= 0) return 0;
    return (size_t)batch * (size_t)((n + 63) / 64) * (size_t)sf_cov_grad_slots(has_global, n_local);
}
int sf_launch_cov_grad(const sf_fill_args& f, int batch, const double* winv, const double* alpha, int ld_alpha, const int* info,
                       double* part, double* grad, int grad_stride, hipStream_t s) {
    SF_CHECK(sf_check_n_local(f));
    sf_grad_args a;
    a.f = f;
    a.winv = winv, a.alpha = alpha, a.ld_alpha = ld_alpha, a.info = info, a.part = part, a.grad = grad, a.grad_stride = grad_stride;
    a.nbr = (f.n + 63) / 64, a.nslots = sf_cov_grad_slots(f.has_global, f.n_local), a.batch = batch;
    if (f.n <= 0 || f.npad % SF_LEAF != 0 || f.npad < f.n || a.nslots < 1 || grad_stride < a.nslots || ld_alpha < f.n || batch < 1 ||
        batch > 65535) {
        sf_set_error("cov grad: n, npad a multiple of %d, a structured kernel, grad_stride >= slots, ld_alpha >= n, batch in 1 .. 65535",
                     SF_LEAF);
        return SF_EINVAL;
    }
    const long long grid = (long long)batch * a.nbr;
    SF_CHECK(sf_check_fill_grid(grid));
    hipLaunchKernelGGL(k_cov_grad, dim3((unsigned)grid), dim3(256), 0, s, a);
    SF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_cov_grad_sum, dim3((a.nslots + 63) / 64, batch), dim3(64), 0, s, a);
    SF_LAUNCH_CHECK();
    return SF_OK;
}
