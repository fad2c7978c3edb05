// The covariance applied to vectors, one component at a time, without materialising a matrix:
//     out[b][k][r][:] = K_k v[b][r][:],   C = sum_k K_k = Y^T Y + diag(sigma^2 + 1e-10) + K_global + sum_j K_local,j
// k = 0 emulator, 1 noise (the likelihood's jitter included: the components sum to C v for the matrix that is factorised),
// 2 global, 3 + j local kernel j.  With v = C^-1 r these are the conditional means of the components given the residual
// (sf_decompose_batch).  A layer of sf_fill.hip: the structured entries come from the fill's own sf_matern_elem /
// sf_local_elem / sf_local_metric with the fill's operands (sf_load_global / sf_load_local) under the same -ffp-contract=off, so an entry
// multiplied here has the bits of the entry the fill adds to C (the per-entry fill: on a log-uniform grid the likelihood's
// fill reads K_global from its per-diagonal table, equal to the rounding of the grid).
//
// Two launches.  k_cov_yv: t = Y v, one workgroup per (walker, right-hand side), a wave per row of Y.  k_cov_matvec: one
// workgroup (4 waves) per (walker, 64-row block, group of up to 16 right-hand sides); lane = row of the block.  Per
// structured component the workgroup walks the 256-column chunks that hold a 64-column block the component can reach
// (sf_block_support, the fill's conservative test; every block on a grid that is not monotonic), stages the chunk of v
// and of the wavelengths in LDS, and wave w takes every fourth column: one evaluated entry serves all right-hand sides
// of the group.  The four partial sums of a row meet in LDS and are added in wave order.  Plain VALU arithmetic: the
// entry (an exp, a cos, a division) costs an order of magnitude more than the up to 16 multiply-adds it feeds, so the
// matrix cores would have nothing to do.  No atomics, every sum in a fixed order (the same bits on every call); no
// workgroup waits for another; rows and columns >= n are neither read nor written.
#pragma once

#define SF_MV_NR 16    // right-hand sides of a group (as k_chol_apply)
#define SF_MV_CH 256   // columns of v staged per step: four 64-column blocks
#define SF_MV_SB 256   // 64-column blocks whose support flags are held at a time (n <= 16384: all of them)

struct sf_matvec_args {
    sf_fill_args f;      // wave, sigma, Y, params and the model's layout, exactly as the fill gets them (C is not used)
    int m;               // rows of Y that exist (f.mpad: rows allocated)
    const double* v;     // [batch][nrhs][ldv], n data rows each
    int ldv, nrhs;
    double* yv;          // [batch][nrhs][m]: Y v
    const int* info;     // [batch]: != 0 -> NaN rows
    double* out;         // [batch][3 + n_local][nrhs][n]
    int ngroups, nblk;
};

__global__ __launch_bounds__(256) void k_cov_yv(const sf_matvec_args a) {
    const int r = blockIdx.x, b = blockIdx.y;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (a.info[b] != 0) return;  // (k_cov_matvec writes NaN and does not read yv)
    const double* __restrict__ vb = a.v + ((int64_t)b * a.nrhs + r) * a.ldv;
    const double* __restrict__ Yb = a.f.Y + (int64_t)b * a.f.mpad * a.f.ldy;
    for (int k = w; k < a.m; k += 4) {
        double s = 0.0;
        for (int j = lane; j < a.f.n; j += 64) s = s + Yb[(int64_t)k * a.f.ldy + j] * vb[j];
        s = sf_wave_sum(s);
        if (lane == 0) a.yv[((int64_t)b * a.nrhs + r) * a.m + k] = s;
    }
}

__global__ __launch_bounds__(256) void k_cov_matvec(const sf_matvec_args a) {
    __shared__ double Vs[SF_MV_NR * SF_MV_CH];  // the chunk of v, [rhs][column]; then the waves' partial sums [wave][rhs][row]
    __shared__ double Ws[SF_MV_CH];             // the chunk of the wavelengths
    __shared__ unsigned s_lmask[SF_MV_SB];      // per 64-column block: the local kernels that reach (row block, column block)
    __shared__ unsigned char s_glob[SF_MV_SB];  // ... and whether the global kernel does
    const sf_fill_args& f = a.f;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int bid = blockIdx.x;
    const int rb = bid % a.nblk, g = (bid / a.nblk) % a.ngroups, b = bid / (a.nblk * a.ngroups);
    const int nr = min(SF_MV_NR, a.nrhs - g * SF_MV_NR), n = f.n;
    const int R0 = rb * 64, i = R0 + lane, rhi = min(R0 + 63, n - 1);
    const bool valid = i < n;
    const int ncomp = 3 + f.n_local;
    const double* __restrict__ vb = a.v + ((int64_t)b * a.nrhs + g * SF_MV_NR) * a.ldv;
    // component k, right-hand side r of the group: n rows
    auto out_at = [&](int k, int r) { return a.out + (((int64_t)b * ncomp + k) * a.nrhs + g * SF_MV_NR + r) * n; };
    if (a.info[b] != 0) {
        for (int k = 0; k < ncomp; ++k)
            for (int r = w; r < nr; r += 4)
                if (valid) out_at(k, r)[i] = __builtin_nan("");
        return;
    }
    // emulator: Y^T (Y v), m terms per row; noise: one rounding for sigma^2 + jitter, one for the product
    {
        const double* __restrict__ Yb = f.Y + (int64_t)b * f.mpad * f.ldy;
        const double* __restrict__ tb = a.yv + ((int64_t)b * a.nrhs + g * SF_MV_NR) * a.m;
        if (valid) {
            const double sg = f.sigma[i];
            const double s2 = __builtin_fma(sg, sg, SF_JITTER);
            for (int r = w; r < nr; r += 4) {
                double e = 0.0;
                for (int k = 0; k < a.m; ++k) e = e + Yb[(int64_t)k * f.ldy + i] * tb[r * a.m + k];
                out_at(0, r)[i] = e;
                out_at(1, r)[i] = s2 * vb[(int64_t)r * a.ldv + i];
                if (!f.has_global) out_at(2, r)[i] = 0.0;
            }
        }
    }
    const double* __restrict__ P = f.params + (int64_t)b * f.pstride;
    sf_global_hyper gh = {0, 1, 0};
    if (f.has_global) gh = sf_load_global(f, P);
    const double w_row = valid ? f.wave[i] : 1.0;
    const int ncb = (n + 63) / 64;
    int flags_of = -1;  // first column block of the support flags in LDS
    for (int c = f.has_global ? 0 : 1; c <= f.n_local; ++c) {  // 0: global, 1 + k: local kernel k
        sf_local_hyper l = {1, 0, 1};
        double d_row = 0;
        if (c > 0) {
            l = sf_load_local(f, P, c - 1);
            d_row = sf_local_metric(w_row, l.mu);
        }
        double acc[SF_MV_NR];
#pragma unroll
        for (int r = 0; r < SF_MV_NR; ++r) acc[r] = 0.0;
        for (int sb0 = 0; sb0 < ncb; sb0 += SF_MV_SB) {
            const int nsb = min(SF_MV_SB, ncb - sb0);
            if (flags_of != sb0) {  // (uniform; once per workgroup while n <= 16384)
                __syncthreads();
                if (tid < nsb) {
                    const int clo = (sb0 + tid) * 64;
                    bool dg;
                    unsigned lm;
                    sf_block_support(f, P, R0, rhi, clo, min(clo + 63, n - 1), gh.r0, dg, lm);
                    s_glob[tid] = dg ? 1 : 0;
                    s_lmask[tid] = lm;
                }
                __syncthreads();
                flags_of = sb0;
            }
            for (int ch = 0; ch < nsb; ch += 4) {
                unsigned hit = 0;  // the blocks of this chunk the component reaches (the same in every thread)
                for (int q = 0; q < 4 && ch + q < nsb; ++q)
                    if (c == 0 ? s_glob[ch + q] != 0 : ((s_lmask[ch + q] >> (c - 1)) & 1u) != 0) hit |= 1u << q;
                if (!hit) continue;
                const int c0 = (sb0 + ch) * 64;
                __syncthreads();  // the last readers of Vs / Ws are done
                for (int e = tid; e < nr * SF_MV_CH; e += 256) {
                    const int r = e / SF_MV_CH, j = c0 + (e % SF_MV_CH);
                    Vs[e] = j < n ? vb[(int64_t)r * a.ldv + j] : 0.0;
                }
                Ws[tid] = c0 + tid < n ? f.wave[c0 + tid] : 1.0;
                __syncthreads();
                for (int q = 0; q < 4; ++q) {
                    if (!((hit >> q) & 1u)) continue;
                    for (int jj = q * 64 + w; jj < q * 64 + 64 && c0 + jj < n; jj += 4) {
                        const double w_col = Ws[jj];
                        const double e = c == 0 ? sf_matern_elem(w_row, w_col, gh.amp, gh.ls, gh.r0)
                                                : sf_local_elem(d_row, sf_local_metric(w_col, l.mu), l.amp, l.sig, 4 * l.sig);
#pragma unroll
                        for (int r = 0; r < SF_MV_NR; ++r)
                            if (r < nr) acc[r] = acc[r] + e * Vs[r * SF_MV_CH + jj];
                    }
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < SF_MV_NR; ++r)
            if (r < nr) Vs[(w * SF_MV_NR + r) * 64 + lane] = acc[r];
        __syncthreads();
        for (int r = w; r < nr; r += 4) {
            double s = Vs[r * 64 + lane];
            for (int ww = 1; ww < 4; ++ww) s = s + Vs[(ww * SF_MV_NR + r) * 64 + lane];
            if (valid) out_at(c == 0 ? 2 : 2 + c, r)[i] = s;
        }
    }
}

int sf_launch_cov_matvec(const sf_fill_args& f, int m, const double* v, int ldv, int nrhs, int batch, double* yv,
                         const int* info, double* out, hipStream_t s) {
    SF_CHECK(sf_check_n_local(f));
    if (f.n <= 0 || m <= 0 || m > f.mpad || ldv < f.n || nrhs < 1 || nrhs > 65535 || batch < 1 || batch > 65535) {
        sf_set_error("cov matvec: n, m <= mpad, ldv >= n, and nrhs, batch in 1 .. 65535");
        return SF_EINVAL;
    }
    sf_matvec_args a;
    a.f = f;
    a.m = m, a.v = v, a.ldv = ldv, a.nrhs = nrhs, a.yv = yv, a.info = info, a.out = out;
    a.ngroups = (nrhs + SF_MV_NR - 1) / SF_MV_NR;
    a.nblk = (f.n + 63) / 64;
    const long long grid = (long long)batch * a.ngroups * a.nblk;
    SF_CHECK(sf_check_fill_grid(grid));
    hipLaunchKernelGGL(k_cov_yv, dim3(nrhs, batch), dim3(256), 0, s, a);
    SF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_cov_matvec, dim3((unsigned)grid), dim3(256), 0, s, a);
    SF_LAUNCH_CHECK();
    return SF_OK;
}
