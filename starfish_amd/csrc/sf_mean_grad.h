// The likelihood's gradient in the mean-flux parameters (vsini, vz, log_scale, Av, cheb:k and the emulator's grid parameters).
// A layer of sf_transform.hip.  With alpha = C^-1 r, V = C^-1 X^T, a = X alpha, z_a = Sigma_w^-1 a, H = X V,
// W = V Sigma_w^-1 and u_ik = alpha_i (z_a,k - mu_k) - W_ik ("Gradient in the mean-flux parameters"):
//   * a parameter that moves the m + 2 raw rows (eig_k, mean, std; X_k = sc eig_k std, f = sc (sum_k mu_k eig_k std + mean))
//     by d eig_k, d mean, d std and leaves Sigma_w alone has
//         d lnL = sum_i [ sc std sum_k d eig_k u_k  +  sc d std sum_k eig_k u_k  -  sc alpha d mean ]
//   * a grid parameter moves mu and Sigma_w = v22 - z^T z (z = Linv v12) and leaves the rows alone:
//         d lnL = -d mu^T a - sum_r sum_k d z_rk (z Q)_rk,      Q = Sigma_w^-1 H Sigma_w^-1 - z_a z_a^T
// Launches: k_mean_stage puts [r, X_1 .. X_m] into the staging area as 1 + m right-hand sides (before the factorisation);
// the tangents that need no solve (sf_launch_mean_tangents: the d / d vsini spline coefficients through k_rot_dmult, the
// unchanged k_broaden_half and sf_launch_spline_apply; d v12, d mu and d z = Linv d v12 through the unchanged k_emu_z); then
// behind the solve (sf_launch_mean_grad) the moments a, H (k_mean_moments), the m x m algebra (k_mean_finish), the pixel
// pass (k_mean_pixel), the grid slots (k_mean_grid) and the sum over the blocks (k_mean_sum).
// No inverse is formed.  Every sum has a fixed order and there are no atomics: a thread owns a pixel, a workgroup sums its
// 256 pixels (xor shuffles, then the four waves in wave order) into part[b][block][slot], and k_mean_sum adds the blocks in
// ascending order -- the frame of sf_grad_frame.h, whose k_grad_sum lives in another translation unit and halves.  A slot's
// arithmetic does not depend on the other slots asked for.  Walkers with info != 0 are not read; their rows come out NaN.
#pragma once
#include "sf_device.h"
#include "sf_transform.h"
#include "sf_transform_emu.h"
#include "sf_transform_eval.h"
#include "sf_transform_fft.h"
#include "sf_transform_spline.h"

// ------------------------------------------------------------------------------------------ tangent pieces
// d h / d x of sf_bspl6's six values (de Boor: B'_{i,5} = 5 [B_{i,4} / (t_{i+5} - t_i) - B_{i+1,4} / (t_{i+6} - t_{i+1})]),
// from the five degree-4 values of the same interval, knots scaled by s as there
__device__ __forceinline__ void sf_bspl6_dx(const double* __restrict__ t, double s, int ell, double x, double dh[6]) {
    double tk[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) tk[i] = t[ell - 5 + i] * s;
    double h[5], hh[4];
    h[0] = 1.0;
#pragma unroll
    for (int j = 1; j <= 4; ++j) {
#pragma unroll
        for (int i = 0; i < j; ++i) hh[i] = h[i];
        h[0] = 0.0;
#pragma unroll
        for (int i = 1; i <= j; ++i) {
            const double tli = tk[5 + i], tlj = tk[5 + i - j];
            const double f = hh[i - 1] / (tli - tlj);
            h[i - 1] = h[i - 1] + f * (tli - x);
            h[i] = f * (x - tlj);
        }
    }
    // h[p] = B_{ell-4+p, 4}(x); the value q of sf_bspl6 belongs to B_{ell-5+q, 5}
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        const double lo = q >= 1 ? h[q - 1] / (tk[5 + q] - tk[q]) : 0.0;
        const double hi = q <= 4 ? h[q] / (tk[6 + q] - tk[q + 1]) : 0.0;
        dh[q] = 5.0 * (lo - hi);
    }
}

// the exponent of sf_ccm89_mult per unit Av: a(x) + b(x) / Rv, so that d mult / d Av = -0.4 ln 10 (a + b / Rv) mult
__device__ __forceinline__ double sf_ccm89_exponent(double wave_A, double Rv) {
    const double x = 1e4 / wave_A;
    double a, b;
    if (x < 1.1) {
        const double p = pow(x, 1.61);
        a = 0.574 * p;
        b = -0.527 * p;
    } else if (x <= 3.3) {
        const double y = x - 1.82;
        a = 1 + y * (0.17699 + y * (-0.50447 + y * (-0.02427 + y * (0.72085 + y * (0.01979 + y * (-0.77530 + y * 0.32999))))));
        b = y * (1.41338 + y * (2.28305 + y * (1.07233 + y * (-5.38434 + y * (-0.62251 + y * (5.30260 + y * -2.09002))))));
    } else if (x <= 8.0) {
        double fa = 0.0, fb = 0.0;
        if (x >= 5.9) {
            const double d = x - 5.9;
            fa = -0.04473 * d * d - 0.009779 * d * d * d;
            fb = 0.2130 * d * d + 0.1207 * d * d * d;
        }
        a = 1.752 - 0.316 * x - 0.104 / ((x - 4.67) * (x - 4.67) + 0.341) + fa;
        b = -3.090 + 1.825 * x + 1.206 / ((x - 4.62) * (x - 4.62) + 0.263) + fb;
    } else {
        const double d = x - 8.0;
        a = -1.073 - 0.628 * d + 0.137 * d * d - 0.070 * d * d * d;
        b = 13.670 + 4.257 * d - 0.420 * d * d + 0.374 * d * d * d;
    }
    return a + b / Rv;
}

// d sb / d vsini of sf_rot_mult's sb(u) = j1(u)/u - 3 cos u / (2 u^2) + 3 sin u / (2 u^3), u = 2 pi vsini k val:
//     u sb'(u) / vsini,   sb'(u) = j0/u - 2 j1/u^2 + 3 sin u / (2 u^2) + 9 cos u / (2 u^3) - 9 sin u / (2 u^4).
// The closed form cancels like 20 eps / u^4; below SF_ROT_DSERIES_U the power series sb = sum_k (-1)^k c_k u^2k,
// c_k = 1 / (2^(2k+1) k! (k+1)!) + 3 (k+1) / (2k+3)!, is differentiated term by term (12 terms).  The switch point comes from
// a comparison of both float64 forms with a 40-term np.longdouble series (tests/test_mean_gradient_host.py repeats it): at
// u = 2 the closed form is within 7e-16 relative and 12 terms within 3e-16; at u = 1.5 the closed form loses 2e-15, at
// u = 2.5 twelve terms still hold 3e-16, at u = 3 they lose 2e-15.
#define SF_ROT_DSERIES_U 2.0
__device__ __forceinline__ double sf_rot_dmult(int k, double val, double vsini) {
    if (k == 0) return 0.0;
    const double u = 2.0 * M_PI * vsini * (k * val);
    if (u < SF_ROT_DSERIES_U) {
        // (-1)^k 2 k c_k, k = 12 .. 1
        const double c[12] = {3.257565160889156e-25,  -1.882238326196125e-22,  9.13686365824605e-20,  -3.6641518702925286e-17,
                              1.1894396195723791e-14, -3.0471062432939795e-12, 5.963801943619652e-10, -8.542031247109372e-08,
                              8.431600228475229e-06,  -0.0005239335317460317,  0.01755952380952381,   -0.225};
        const double u2 = u * u;
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < 12; ++i) s = s * u2 + c[i];
        return s * u2 / vsini;  // (s u^2 = u sb'(u))
    }
    const double u2 = u * u, sn = sin(u), cs = cos(u);
    const double d = j0(u) / u - 2.0 * j1(u) / u2 + 3.0 * sn / (2.0 * u2) + 9.0 * cs / (2.0 * (u2 * u)) - 9.0 * sn / (2.0 * (u2 * u2));
    return d * u / vsini;
}
// mult[b][k] = d sb_k / d vsini of walker b (k_kernel_mult's table for the tangent rows); walkers with vsini <= 0 were
// flagged by k_kernel_mult and are skipped by k_broaden_half
__global__ __launch_bounds__(256) void k_rot_dmult(double* __restrict__ mult, int nh1, double val,
                                                   const double* __restrict__ params, int pstride) {
    const int b = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
    const double vsini = params[(int64_t)b * pstride];
    if (k >= nh1 || !(vsini > 0.0)) return;
    mult[(int64_t)b * nh1 + k] = sf_rot_dmult(k, val, vsini);
}

// d v12 / d theta_p per block (k_i[j] (g_jp - theta_p) / l_ip^2 from the k_i[j] k_emu_prep left) and d mu_i = d v12_i^T alpha_i.
// grid (B, ng): workgroup (b, g) serves the g-th grid column asked for
__global__ __launch_bounds__(256) void k_mean_emu_dk(const sf_emu_args e, const sf_mean_grad_args a, int B) {
    __shared__ double red[4];
    const int b = blockIdx.x, g = blockIdx.y, tid = threadIdx.x;
    const int mM = e.m * e.M, p = a.gcols[g] - e.off_grid;
    const double th = e.params[(int64_t)b * e.pstride + e.off_grid + p];
    const double* __restrict__ kv = e.kbuf + (int64_t)b * mM;
    double* __restrict__ kd = a.kdot + ((int64_t)g * B + b) * mM;
    for (int q = tid; q < mM; q += 256) {
        const int i = q / e.M, j = q - i * e.M;
        const double l = e.lengthscales[i * e.P + p];
        kd[q] = kv[q] * ((e.grid[j * e.P + p] - th) / (l * l));
    }
    __syncthreads();
    for (int i = 0; i < e.m; ++i) {
        double acc = 0.0;
        for (int j = tid; j < e.M; j += 256) acc += kd[i * e.M + j] * e.alpha[i * e.M + j];
        acc = sf_block_sum(acc, red);
        if (tid == 0) a.mudot[((int64_t)g * B + b) * e.m + i] = acc;
    }
}

// the launches that need no solve: a.dcoef (want_vsini) and a.kdot / a.mudot / a.zdot (ng grid columns; a.zdot only with want_zdot:
// the Fisher columns read d mu alone).  bro: the broadening's
// arguments as run_transforms filled them (its ybro, mult and FFT scratch are free again and are used once more)
int sf_launch_mean_tangents(const sf_broaden_args& bro, const double* inv_band, const sf_emu_args& e, const sf_mean_grad_args& a,
                            int B, hipStream_t s, bool want_zdot) {
    if (a.want_vsini) {
        const int nh1 = bro.nf / 2 + 1;
        hipLaunchKernelGGL(k_rot_dmult, dim3((nh1 + 255) / 256, B), dim3(256), 0, s, bro.mult, nh1, 1.0 / (bro.nf * bro.dv), bro.params,
                           bro.pstride);
        SF_LAUNCH_CHECK();
        SF_CHECK(launch_broaden_half_rows(bro, s));
        SF_CHECK(sf_launch_spline_apply(bro.out, a.dcoef, B, bro.rows, bro.nf, inv_band, s));
    }
    if (a.ng > 0) {
        hipLaunchKernelGGL(k_mean_emu_dk, dim3(B, a.ng), dim3(256), 0, s, e, a, B);
        SF_LAUNCH_CHECK();
        const int mM = e.m * e.M;
        for (int g = 0; want_zdot && g < a.ng; ++g) {  // d z = Linv d v12: the emulator's own product on the tangent blocks
            sf_emu_args t = e;
            t.kbuf = a.kdot + (int64_t)g * B * mM;
            t.zscratch = a.zdot + (int64_t)g * B * mM * e.m;
            hipLaunchKernelGGL(k_emu_z, dim3((mM + 255) / 256, e.m, (B + EMU_WCHUNK - 1) / EMU_WCHUNK), dim3(256),
                               sizeof(double) * (size_t)EMU_WCHUNK * e.M, s, t, B);
            SF_LAUNCH_CHECK();
        }
    }
    return SF_OK;
}

// ------------------------------------------------------------------------------------------ staging
// stage[b][0][0:npad) = the walker's residual, stage[b][1 + k] = its scaled row X_k, zero on the padding; all zero for a
// walker the transform chain flagged (its X was never written)
__global__ void k_mean_stage(const double* __restrict__ resid, const double* __restrict__ Xs, const int* __restrict__ info,
                             int n, int npad, int m, double* __restrict__ stage) {
    const int r = blockIdx.y, b = blockIdx.z;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npad) return;
    double v = 0.0;
    if (i < n && info[b] == 0) v = r == 0 ? resid[(int64_t)b * npad + i] : Xs[((int64_t)b * m + (r - 1)) * n + i];
    stage[((int64_t)b * (1 + m) + r) * npad + i] = v;
}
int sf_launch_mean_stage(const double* resid, const double* Xs, const int* info, int n, int npad, int m, int batch, double* stage,
                         hipStream_t s) {
    hipLaunchKernelGGL(k_mean_stage, dim3((npad + 255) / 256, 1 + m, batch), dim3(256), 0, s, resid, Xs, info, n, npad, m, stage);
    SF_LAUNCH_CHECK();
    return SF_OK;
}

// ------------------------------------------------------------------------------------------ behind the solve
// fin[b]: z_a (m), Sigma_w^-1 (m x m), Q (m x m; Lw^-1 on the way), a (m), H (m x m)
__device__ __forceinline__ double* sf_mean_fin(const sf_mean_grad_args& a, int b) { return a.fin + (int64_t)b * sf_mean_fin_doubles(a.m); }

// workgroup (k, b): a_k = X_k . alpha and, for the grid slots, H_kl = X_k . V_l; the pixels strided over the threads
__global__ __launch_bounds__(256) void k_mean_moments(const sf_mean_grad_args a) {
    __shared__ double red[4];
    const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, m = a.m;
    if (a.info[b] != 0) return;
    const double* __restrict__ st = a.stage + (int64_t)b * (1 + m) * a.npad;
    const double* __restrict__ Xk = a.Xs + ((int64_t)b * m + k) * a.n;
    double* __restrict__ fin = sf_mean_fin(a, b);
    for (int l = 0; l <= (a.ng > 0 ? m : 0); ++l) {
        const double* __restrict__ v = st + (int64_t)l * a.npad;
        double acc = 0.0;
        for (int i = tid; i < a.n; i += 256) acc = acc + Xk[i] * v[i];
        acc = sf_block_sum(acc, red);
        if (tid == 0) fin[m + 2 * m * m + (l == 0 ? k : m + k * m + (l - 1))] = acc;
    }
}
// one thread per walker: Sigma_w^-1 = Lw^-T Lw^-1, z_a = Sigma_w^-1 a and, for the grid slots, Q = Sigma_w^-1 H Sigma_w^-1 - z_a z_a^T
__global__ void k_mean_finish(const sf_mean_grad_args a, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x, m = a.m;
    if (b >= B || a.info[b] != 0) return;
    const double* __restrict__ Lw = a.Lw + (int64_t)b * m * m;
    double* __restrict__ za = sf_mean_fin(a, b);
    double* __restrict__ Si = za + m;
    double* __restrict__ Q = Si + m * m;  // Lw^-1 first
    const double* __restrict__ av = Q + m * m;
    const double* __restrict__ H = av + m;
    for (int c = 0; c < m; ++c)  // column c of Lw^-1 by forward substitution
        for (int r = 0; r < m; ++r) {
            double v = r == c ? 1.0 : 0.0;
            for (int j = c; j < r; ++j) v = v - Lw[r * m + j] * Q[j * m + c];
            Q[r * m + c] = r < c ? 0.0 : v / Lw[r * m + r];
        }
    for (int r = 0; r < m; ++r)
        for (int c = 0; c <= r; ++c) {
            double v = 0.0;
            for (int j = r; j < m; ++j) v = v + Q[j * m + r] * Q[j * m + c];
            Si[r * m + c] = v;
            Si[c * m + r] = v;
        }
    for (int k = 0; k < m; ++k) {
        double v = 0.0;
        for (int l = 0; l < m; ++l) v = v + Si[k * m + l] * av[l];
        za[k] = v;
    }
    if (a.ng == 0) return;
    // Q = Si H Si - za za^T, row by row through one row of Si H
    double t[SF_MAX_M];
    for (int r = 0; r < m; ++r) {
        for (int c = 0; c < m; ++c) {
            double v = 0.0;
            for (int j = 0; j < m; ++j) v = v + Si[r * m + j] * H[j * m + c];
            t[c] = v;
        }
        for (int c = 0; c < m; ++c) {
            double v = 0.0;
            for (int j = 0; j < m; ++j) v = v + t[j] * Si[j * m + c];
            Q[r * m + c] = v - za[r] * za[c];
        }
    }
}

// One thread per pixel.  With the rows before the Chebyshev multiply (e_k, mean0, std0: spline value times extinction), p the
// Chebyshev series,  A' = sc p std0 sum_k e_k u_k  and  M' = -sc alpha mean0:
//     log_scale: p (A' + M')     cheb:k: T_k (2 A' + M')     Av: -0.4 ln 10 (a + b / Rv) p (2 A' + M')
// (a factor common to all m + 2 rows enters eig_k and std: the 2), and with d_r a tangent of row r before the Chebyshev multiply
//     sc p^2 (std0 sum_k d_k u_k + d_std sum_k e_k u_k) - sc p alpha d_mean
// for vsini (d_r: the spline of the d / d vsini coefficients times the extinction) and, times -x c / (c^2 - vz^2), for vz (d_r:
// the x-derivative of row r's spline in the scaled-knot frame times the extinction).  Grid columns are k_mean_grid's.
__global__ __launch_bounds__(256) void k_mean_pixel(const sf_eval_args e, const sf_mean_grad_args a) {
    __shared__ double red[4];
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y, m = a.m;
    if (a.info[b] != 0) return;  // (uniform over the workgroup)
    double Ap = 0.0, Mp = 0.0, Vz = 0.0, Vs = 0.0, p = 1.0, x = 1.0;
    const double* __restrict__ P = e.params + (int64_t)b * e.pstride;
    if (i < a.n) {
        x = e.wave[i];
        double s = 1.0, vz = 0.0;
        if (e.has_vz) {
            vz = P[1];
            s = sqrt((SF_C_KMS + vz) / (SF_C_KMS - vz));
        }
        const int ell = sf_find_interval(e.knots, s, e.nf, x);
        double h[6], dh[6];
        sf_bspl6(e.knots, s, ell, x, h);
        if (a.want_vz) sf_bspl6_dx(e.knots, s, ell, x, dh);
        const int rows = m + 2;
        const int64_t coff = (e.coef_batched ? (int64_t)b * e.nf * rows : 0) + (int64_t)(ell - 5) * rows;
        const double* __restrict__ cf = e.coef + coff;
        const double* __restrict__ dcf = a.want_vsini ? a.dcoef + coff : cf;
        if (e.n_cheb > 0) p = sf_chebval(x / e.wave_max, P + e.off_cheb, e.n_cheb + 1, 1.0);
        double ext = 1.0;
        if (e.has_av) ext = sf_ccm89_mult(x, P[e.off_av], 3.1);
        auto row0 = [&](const double* __restrict__ c6, int r, const double* w6) {  // a spline of row r times the extinction
            double sp = 0.0;
#pragma unroll
            for (int j = 0; j < 6; ++j) sp = sp + c6[(int64_t)j * rows + r] * w6[j];
            return e.has_av ? sp * ext : sp;
        };
        const double* __restrict__ st = a.stage + (int64_t)b * (1 + m) * a.npad + i;
        const double* __restrict__ za = sf_mean_fin(a, b);
        const double* __restrict__ Si = za + m;
        const double* __restrict__ mu = a.mu + (int64_t)b * m;
        const double sc = a.scale[b], alpha = st[0];
        double eu = 0.0, du = 0.0, gu = 0.0;  // sum_k e_k u_k, and the same with the vz / vsini tangents of e_k
        for (int k = 0; k < m; ++k) {
            double w = 0.0;
            for (int l = 0; l < m; ++l) w = w + Si[k * m + l] * st[(int64_t)(1 + l) * a.npad];
            const double u = alpha * (za[k] - mu[k]) - w;
            eu = eu + row0(cf, k, h) * u;
            if (a.want_vz) du = du + row0(cf, k, dh) * u;
            if (a.want_vsini) gu = gu + row0(dcf, k, h) * u;
        }
        const double mean0 = row0(cf, m, h), std0 = row0(cf, m + 1, h);
        Ap = sc * p * std0 * eu;
        Mp = -(sc * alpha * mean0);
        if (a.want_vz) {
            const double q = -(x * SF_C_KMS / (SF_C_KMS * SF_C_KMS - vz * vz));
            Vz = q * (sc * p * p * (std0 * du + row0(cf, m + 1, dh) * eu) - sc * p * alpha * row0(cf, m, dh));
        }
        if (a.want_vsini) Vs = sc * p * p * (std0 * gu + row0(dcf, m + 1, h) * eu) - sc * p * alpha * row0(dcf, m, h);
    }
    double* __restrict__ part = a.part + ((int64_t)b * gridDim.x + blockIdx.x) * a.nslots;
    for (int j = 0; j < a.nslots; ++j) {
        const int col = a.slots[j];
        if (col >= 6 && col < e.off_cheb) continue;  // a grid column
        double v;
        if (col == 0) v = Vs;
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
        v = sf_block_sum(v, red);
        if (threadIdx.x == 0) part[j] = v;
    }
}
// workgroup (b, g): the g-th grid column's slot, -d mu^T a - sum_r sum_k d z_rk (z Q)_rk with the rows r of z strided over the
// threads, into block 0 of the slot's partial sums (zero in the other blocks)
__global__ __launch_bounds__(256) void k_mean_grid(const sf_mean_grad_args a, const double* __restrict__ z, int mM, int B, int nblk) {
    __shared__ double red[4];
    const int b = blockIdx.x, g = blockIdx.y, tid = threadIdx.x, m = a.m;
    if (a.info[b] != 0) return;
    const double* __restrict__ Q = sf_mean_fin(a, b) + m + m * m;
    const double* __restrict__ av = Q + m * m;
    const double* __restrict__ zb = z + (int64_t)b * mM * m;
    const double* __restrict__ zd = a.zdot + ((int64_t)g * B + b) * mM * m;
    double acc = 0.0;
    for (int r = tid; r < mM; r += 256)
        for (int k = 0; k < m; ++k) {
            double zq = 0.0;
            for (int l = 0; l < m; ++l) zq = zq + zb[(int64_t)r * m + l] * Q[l * m + k];
            acc = acc + zd[(int64_t)r * m + k] * zq;
        }
    acc = sf_block_sum(acc, red);
    if (tid != 0) return;
    const double* __restrict__ md = a.mudot + ((int64_t)g * B + b) * m;
    double ma = 0.0;
    for (int k = 0; k < m; ++k) ma = ma + md[k] * av[k];
    int j = 0;
    while (a.slots[j] != a.gcols[g]) ++j;
    for (int I = 0; I < nblk; ++I) a.part[((int64_t)b * nblk + I) * a.nslots + j] = I == 0 ? -ma - acc : 0.0;
}
// grad[b][j] = the blocks' sums in ascending order, NaN where info != 0 (k_grad_sum without its 1/2)
__global__ void k_mean_sum(const sf_mean_grad_args a, int nblk) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (j >= a.nslots) return;
    double s = 0.0;
    if (a.info[b] != 0) {
        s = __builtin_nan("");
    } else {
        for (int I = 0; I < nblk; ++I) s = s + a.part[((int64_t)b * nblk + I) * a.nslots + j];
    }
    a.grad[(int64_t)b * a.grad_stride + j] = s;
}
size_t sf_mean_grad_part_doubles(int n, int nslots, int batch) { return (size_t)batch * ((n + 255) / 256) * (size_t)nslots; }
int sf_launch_mean_grad(const sf_eval_args& e, const sf_mean_grad_args& a, const double* z, int mM, int batch, hipStream_t s) {
    if (a.m > SF_MAX_M || a.nslots < 1 || a.nslots > SF_MEAN_GRAD_MAX_SLOTS) {
        sf_set_error("mean gradient: m=%d / nslots=%d not supported", a.m, a.nslots);
        return SF_EINVAL;
    }
    const int nblk = (a.n + 255) / 256;
    hipLaunchKernelGGL(k_mean_moments, dim3(a.m, batch), dim3(256), 0, s, a);
    SF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mean_finish, dim3((batch + 63) / 64), dim3(64), 0, s, a, batch);
    SF_LAUNCH_CHECK();
    if (a.nslots > a.ng) {
        hipLaunchKernelGGL(k_mean_pixel, dim3(nblk, batch), dim3(256), 0, s, e, a);
        SF_LAUNCH_CHECK();
    }
    if (a.ng > 0) {
        hipLaunchKernelGGL(k_mean_grid, dim3(batch, a.ng), dim3(256), 0, s, a, z, mM, batch, nblk);
        SF_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_mean_sum, dim3((a.nslots + 63) / 64, batch), dim3(64), 0, s, a, nblk);
    SF_LAUNCH_CHECK();
    return SF_OK;
}
