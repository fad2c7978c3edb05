// The Fisher information of the mean-flux parameters at fixed covariance, F_ij = fdot_i^T C^-1 fdot_j, fdot_j = d f / d theta_j
// (the Gauss-Newton block: the term 1/2 tr(C^-1 dC_i C^-1 dC_j) that arises because X sits inside C_emu is left out; the block
// of the covariance hyper-parameters, where that term is all there is, is sf_fisher_cov.h's).
// A layer of sf_transform.hip ("Fisher information in the mean-flux parameters"):
//   columns    k_fisher_tangent: one thread per pixel writes fdot_j(i) of every requested slot into rows of npad doubles, zero
//              on the padding and for a walker the transform chain flagged.  The formulas are k_mean_pixel's with omega = 0 and
//              alpha = -1 (u_k = mu_k, M' = sc mean0); a grid column is mudot^T X.  The per-pixel evaluation is RESTATED here,
//              not shared with k_mean_pixel: that kernel stays instruction for instruction what it was.
//   band       k_fisher_rows stages [r; Y] in front of the columns; the sweep's Gram matrix G of [r; Y; J] then gives
//              k_fisher_lead (the leading (1 + m)^2 block, compact, for the likelihood's capacitance step) and k_fisher_band:
//              S = I + G_YY = L_S L_S^T as k_woodbury factorises it, U = L_S^-1 G_YJ riding along, F = G_JJ - U^T U.
//   dense      Z = L^-1 J in the staging area, then F = Z^T Z: k_fisher_ztz (256-pixel blocks into part[b][block][pair]) and
//              k_fisher_sum (the blocks in ascending order), the frame of sf_grad_frame.h.
// Every sum has one order and there are no atomics; only the lower triangle is computed, the upper one is its mirror, so F_ij
// and F_ji are the same bits.  No register array is indexed by the slot: the slots are a run-time loop.
#pragma once
#include "sf_mean_grad.h"

// ------------------------------------------------------------------------------------------ tangent columns
// rows[b * rstride + j * npad + i] = d f_i / d theta_{slots[j]}, i < npad.  a.info: the transform chain's status (the
// factorisation's is not known yet)
__global__ __launch_bounds__(256) void k_fisher_tangent(const sf_eval_args e, const sf_mean_grad_args a, double* __restrict__ rows,
                                                        int64_t rstride, int B) {
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y, m = a.m;
    if (i >= a.npad) return;
    double* __restrict__ out = rows + (int64_t)b * rstride + i;
    if (i >= a.n || a.info[b] != 0) {
        for (int j = 0; j < a.nslots; ++j) out[(int64_t)j * a.npad] = 0.0;
        return;
    }
    const double* __restrict__ P = e.params + (int64_t)b * e.pstride;
    const double x = e.wave[i];
    double s = 1.0, vz = 0.0, p = 1.0;
    if (e.has_vz) {
        vz = P[1];
        s = sqrt((SF_C_KMS + vz) / (SF_C_KMS - vz));
    }
    const int ell = sf_find_interval(e.knots, s, e.nf, x);
    double h[6], dh[6];
    sf_bspl6(e.knots, s, ell, x, h);
    if (a.want_vz) sf_bspl6_dx(e.knots, s, ell, x, dh);
    const int nrow = m + 2;
    const int64_t coff = (e.coef_batched ? (int64_t)b * e.nf * nrow : 0) + (int64_t)(ell - 5) * nrow;
    const double* __restrict__ cf = e.coef + coff;
    const double* __restrict__ dcf = a.want_vsini ? a.dcoef + coff : cf;
    if (e.n_cheb > 0) p = sf_chebval(x / e.wave_max, P + e.off_cheb, e.n_cheb + 1, 1.0);
    double ext = 1.0;
    if (e.has_av) ext = sf_ccm89_mult(x, P[e.off_av], 3.1);
    auto row0 = [&](const double* __restrict__ c6, int r, const double* w6) {  // a spline of row r times the extinction
        double sp = 0.0;
#pragma unroll
        for (int j = 0; j < 6; ++j) sp = sp + c6[(int64_t)j * nrow + r] * w6[j];
        return e.has_av ? sp * ext : sp;
    };
    const double* __restrict__ mu = a.mu + (int64_t)b * m;
    const double sc = a.scale[b];
    double eu = 0.0, du = 0.0, gu = 0.0;  // sum_k e_k mu_k, and the same with the vz / vsini tangents of e_k
    for (int k = 0; k < m; ++k) {
        const double u = mu[k];
        eu = eu + row0(cf, k, h) * u;
        if (a.want_vz) du = du + row0(cf, k, dh) * u;
        if (a.want_vsini) gu = gu + row0(dcf, k, h) * u;
    }
    const double mean0 = row0(cf, m, h), std0 = row0(cf, m + 1, h);
    const double Ap = sc * p * std0 * eu, Mp = sc * mean0;
    double Vz = 0.0, Vs = 0.0;
    if (a.want_vz) {
        const double q = -(x * SF_C_KMS / (SF_C_KMS * SF_C_KMS - vz * vz));
        Vz = q * (sc * p * p * (std0 * du + row0(cf, m + 1, dh) * eu) + sc * p * row0(cf, m, dh));
    }
    if (a.want_vsini) Vs = sc * p * p * (std0 * gu + row0(dcf, m + 1, h) * eu) + sc * p * row0(dcf, m, h);
    int g = 0;  // grid columns met so far: a.gcols lists them in slot order
    for (int j = 0; j < a.nslots; ++j) {
        const int col = a.slots[j];
        double v;
        if (col >= 6 && col < e.off_cheb) {  // a grid column: mudot^T X
            const double* __restrict__ md = a.mudot + ((int64_t)g * B + b) * m;
            const double* __restrict__ X = a.Xs + (int64_t)b * m * a.n + i;
            v = 0.0;
            for (int k = 0; k < m; ++k) v = v + md[k] * X[(int64_t)k * a.n];
            ++g;
        } else if (col == 0) v = Vs;
        else if (col == 1) v = Vz;
        else if (col == 2) v = p * (Ap + Mp);
        else if (e.has_av && col == e.off_av) v = -0.4 * 2.302585092994046 * sf_ccm89_exponent(x, 3.1) * (p * (2.0 * Ap + Mp));
        else {  // cheb: column off_cheb + pos multiplies T_{pos + 1}(x / wave_max)
            const int deg = col - e.off_cheb + 1;
            const double xc = x / e.wave_max;
            double t0 = 1.0, t1 = xc;
            for (int d = 2; d <= deg; ++d) {
                const double t2 = 2.0 * xc * t1 - t0;
                t0 = t1, t1 = t2;
            }
            v = t1 * (2.0 * Ap + Mp);
        }
        out[(int64_t)j * a.npad] = v;
    }
}
int sf_launch_fisher_tangents(const sf_eval_args& e, const sf_mean_grad_args& a, double* rows, int64_t rstride, int batch,
                              hipStream_t s) {
    if (a.m > SF_MAX_M || a.nslots < 1 || a.nslots > SF_MEAN_GRAD_MAX_SLOTS || !rows || rstride < (int64_t)a.nslots * a.npad) {
        sf_set_error("fisher tangents: m=%d / nslots=%d / rows not supported", a.m, a.nslots);
        return SF_EINVAL;
    }
    hipLaunchKernelGGL(k_fisher_tangent, dim3((a.npad + 255) / 256, batch), dim3(256), 0, s, e, a, rows, rstride, batch);
    SF_LAUNCH_CHECK();
    return SF_OK;
}

// ------------------------------------------------------------------------------------------ band + Woodbury
// buf[b][0] = the walker's residual (zero on the padding), buf[b][1 + k] = row k of Y as the transform chain left it; rows of
// npad doubles, nin rows per walker (the columns J follow behind: k_fisher_tangent)
__global__ __launch_bounds__(256) void k_fisher_rows(const double* __restrict__ resid, const double* __restrict__ Y, int64_t sy, int n,
                                                     int npad, int nin, double* __restrict__ buf) {
    const int r = blockIdx.y, b = blockIdx.z;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= npad) return;
    double v = 0.0;
    if (r >= 1) v = Y[(int64_t)b * sy + (int64_t)(r - 1) * npad + i];
    else if (i < n) v = resid[(int64_t)b * npad + i];
    buf[((int64_t)b * nin + r) * npad + i] = v;
}
int sf_launch_fisher_rows(const double* resid, const double* Y, int64_t sy, int n, int npad, int m, int nin, int batch, double* buf,
                          hipStream_t s) {
    if (!resid || !Y || !buf || n <= 0 || npad < n || m < 1 || nin < 1 + m || batch <= 0 || batch > 65535) {
        sf_set_error("fisher rows: bad arguments (n=%d npad=%d, %d of %d rows, batch=%d)", n, npad, 1 + m, nin, batch);
        return SF_EINVAL;
    }
    hipLaunchKernelGGL(k_fisher_rows, dim3((npad + 255) / 256, 1 + m, batch), dim3(256), 0, s, resid, Y, sy, n, npad, nin, buf);
    SF_LAUNCH_CHECK();
    return SF_OK;
}
// lead[b] = the leading nl x nl block of gram[b] (nin x nin), compact: what sf_launch_woodbury takes
__global__ __launch_bounds__(64) void k_fisher_lead(const double* __restrict__ gram, int nin, int nl, double* __restrict__ lead) {
    const int b = blockIdx.x;
    const double* __restrict__ g = gram + (int64_t)b * nin * nin;
    double* __restrict__ o = lead + (int64_t)b * nl * nl;
    for (int e = threadIdx.x; e < nl * nl; e += 64) o[e] = g[(e / nl) * nin + (e % nl)];
}
// One wave per walker.  gram[b]: the (1 + m + p)^2 Gram matrix of [r; Y; J].  S = I + G_YY is factorised column by column as in
// k_woodbury, the forward substitution of the p columns of G_YJ riding along (lane c < p owns column c of U); then the lower
// triangle of G_JJ - U^T U, the sum over k ascending, mirrored.  info: the call's final status; != 0 -> a NaN matrix.
__global__ __launch_bounds__(64) void k_fisher_band(const double* __restrict__ gram, int m, int p, const int* __restrict__ info,
                                                    double* __restrict__ fisher, int64_t fstride) {
    __shared__ double S[SF_MAX_M * (SF_MAX_M + 1)];
    __shared__ double U[SF_MAX_M * SF_MEAN_GRAD_MAX_SLOTS];
    const int b = blockIdx.x, lane = threadIdx.x, nin = 1 + m + p, LD = SF_MAX_M + 1;
    double* __restrict__ F = fisher + (int64_t)b * fstride;
    if (info[b] != 0) {  // (uniform over the wave)
        for (int e = lane; e < p * p; e += 64) F[e] = __builtin_nan("");
        return;
    }
    const double* __restrict__ g = gram + (int64_t)b * nin * nin;
    for (int e = lane; e < m * m; e += 64) {
        const int r = e / m, c = e - r * m;
        S[r * LD + c] = g[(r + 1) * nin + (c + 1)] + (r == c ? 1.0 : 0.0);
    }
    for (int e = lane; e < m * p; e += 64) {
        const int r = e / p, c = e - r * p;
        U[r * SF_MEAN_GRAD_MAX_SLOTS + c] = g[(r + 1) * nin + (1 + m + c)];
    }
    __syncthreads();
    for (int j = 0; j < m; ++j) {
        const double rs = 1.0 / sqrt(S[j * LD + j]);  // (a pivot <= 0 was flagged by the capacitance step: not reached)
        __syncthreads();
        double lij = 0.0;
        if (lane > j && lane < m) {
            lij = S[lane * LD + j] * rs;
            S[lane * LD + j] = lij;
        }
        if (lane < p) U[j * SF_MEAN_GRAD_MAX_SLOTS + lane] *= rs;  // u_j = (g_j - sum_{k<j} l_jk u_k) / l_jj
        __syncthreads();
        if (lane > j && lane < m)
            for (int c = j + 1; c <= lane; ++c) S[lane * LD + c] -= lij * S[c * LD + j];
        if (lane < p)  // column `lane` of the rows below j, with the l_rj the lanes r > j have just stored
            for (int r = j + 1; r < m; ++r) U[r * SF_MEAN_GRAD_MAX_SLOTS + lane] -= S[r * LD + j] * U[j * SF_MEAN_GRAD_MAX_SLOTS + lane];
        __syncthreads();
    }
    for (int e = lane; e < p * (p + 1) / 2; e += 64) {
        int i = 0;
        while ((i + 1) * (i + 2) / 2 <= e) ++i;
        const int jc = e - i * (i + 1) / 2;
        double uu = 0.0;
        for (int k = 0; k < m; ++k) uu = uu + U[k * SF_MEAN_GRAD_MAX_SLOTS + i] * U[k * SF_MEAN_GRAD_MAX_SLOTS + jc];
        const double v = g[(1 + m + i) * nin + (1 + m + jc)] - uu;
        F[i * p + jc] = v;
        F[jc * p + i] = v;
    }
}
int sf_launch_fisher_lead(const double* gram, int nin, int nl, int batch, double* lead, hipStream_t s) {
    hipLaunchKernelGGL(k_fisher_lead, dim3(batch), dim3(64), 0, s, gram, nin, nl, lead);
    SF_LAUNCH_CHECK();
    return SF_OK;
}
int sf_launch_fisher_band(const double* gram, int m, int p, int batch, const int* info, double* fisher, int64_t fstride,
                          hipStream_t s) {
    if (m < 1 || m > SF_MAX_M || p < 1 || p > SF_MEAN_GRAD_MAX_SLOTS || fstride < (int64_t)p * p) {
        sf_set_error("fisher band: m=%d / nslots=%d / stride not supported", m, p);
        return SF_EINVAL;
    }
    hipLaunchKernelGGL(k_fisher_band, dim3(batch), dim3(64), 0, s, gram, m, p, info, fisher, fstride);
    SF_LAUNCH_CHECK();
    return SF_OK;
}

// ------------------------------------------------------------------------------------------ dense factor
// part[b][block][pair(i >= j)] = the block's sum over its 256 pixels of Z_i Z_j (xor shuffles, then the four waves in wave
// order); Z: [B][p][npad], the staging area after SF_APPLY_LINV.  Walkers with info != 0 are not read.
__global__ __launch_bounds__(256) void k_fisher_ztz(const double* __restrict__ Z, int n, int npad, int p, const int* __restrict__ info,
                                                    double* __restrict__ part) {
    __shared__ double red[4];
    const int px = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (info[b] != 0) return;  // (uniform over the workgroup)
    const double* __restrict__ z = Z + (int64_t)b * p * npad + px;
    double* __restrict__ o = part + ((int64_t)b * gridDim.x + blockIdx.x) * (p * (p + 1) / 2);
    for (int i = 0; i < p; ++i) {
        const double zi = px < n ? z[(int64_t)i * npad] : 0.0;
        for (int j = 0; j <= i; ++j) {
            double v = px < n ? zi * z[(int64_t)j * npad] : 0.0;
            v = sf_block_sum(v, red);
            if (threadIdx.x == 0) o[i * (i + 1) / 2 + j] = v;
        }
    }
}
// fisher[b][i][j] = fisher[b][j][i] = the blocks' sums in ascending order; NaN where info != 0
__global__ void k_fisher_sum(const double* __restrict__ part, int nblk, int p, const int* __restrict__ info,
                             double* __restrict__ fisher, int64_t fstride) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y, npair = p * (p + 1) / 2;
    if (e >= npair) return;
    int i = 0;
    while ((i + 1) * (i + 2) / 2 <= e) ++i;
    const int j = e - i * (i + 1) / 2;
    double s = 0.0;
    if (info[b] != 0) {
        s = __builtin_nan("");
    } else {
        for (int I = 0; I < nblk; ++I) s = s + part[((int64_t)b * nblk + I) * npair + e];
    }
    double* __restrict__ F = fisher + (int64_t)b * fstride;
    F[i * p + j] = s;
    F[j * p + i] = s;
}
size_t sf_fisher_part_doubles(int n, int nslots, int batch) {
    return (size_t)batch * ((n + 255) / 256) * ((size_t)nslots * (nslots + 1) / 2);
}
int sf_launch_fisher_ztz(const double* Z, int n, int npad, int p, int batch, const int* info, double* part, double* fisher,
                         int64_t fstride, hipStream_t s) {
    if (p < 1 || p > SF_MEAN_GRAD_MAX_SLOTS || fstride < (int64_t)p * p) {
        sf_set_error("fisher ztz: nslots=%d / stride not supported", p);
        return SF_EINVAL;
    }
    const int nblk = (n + 255) / 256;
    hipLaunchKernelGGL(k_fisher_ztz, dim3(nblk, batch), dim3(256), 0, s, Z, n, npad, p, info, part);
    SF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_fisher_sum, dim3((p * (p + 1) / 2 + 63) / 64, batch), dim3(64), 0, s, part, nblk, p, info, fisher, fstride);
    SF_LAUNCH_CHECK();
    return SF_OK;
}
