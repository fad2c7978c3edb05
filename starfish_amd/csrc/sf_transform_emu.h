// The emulator: GP conditional of the PCA weights per walker (k_emu_prep/z/post), the joint conditional over several
// query points (k_emu_joint), and the last step of the likelihood (k_finish).   Starfish/emulator/emulator.py:330-394
#pragma once
#include "sf_device.h"
#include "sf_transform.h"
#include "sf_transform_eval.h"  // sf_block_sum

// ------------------------------------------------------------------------------------ emulator
// emulator.py:376-388 with the constant v11 factored once:
//   v11 = Lc Lc^T, alpha = v11^-1 w_hat, Linv = Lc^-1 (lower);  z = Linv v12;
//   mu = v12^T alpha;  cov = v22 - z^T z.   Also returns Lw = chol(cov) for the rank-m factor.
// Three launches for the whole batch:
//   k_emu_prep   per walker: range check, the v12 blocks k_i[j] (kernels.py:25-26) -> kbuf, mu
//   k_emu_z      z[b][r][i] = sum_j Linv[r][i M + j] k_i[b][j] as a TILED product: a workgroup owns 256 rows r of one
//                component i and 8 walkers; Linv^T is stored (row index fastest) so that the lanes read it coalesced,
//                every element loaded once serves 8 walkers from registers, the k_i of the 8 walkers sit in LDS.
//                (One workgroup per walker streaming its own copy of Linv -- 13.9 MB at the reference's worked
//                example m = 4, M = 330 -- took 0.5 ms per 128 walkers.)
//   k_emu_post   per walker: cov = v22 - z^T z, chol(cov)
#define EMU_WCHUNK 8
__global__ __launch_bounds__(256) void k_emu_prep(sf_emu_args a) {
    __shared__ int bad;
    __shared__ double red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const double* __restrict__ P = a.params + (int64_t)b * a.pstride + a.off_grid;
    const int mM = a.m * a.M;
    if (tid == 0) {
        bad = 0;
        for (int d = 0; d < a.P; ++d)
            if (P[d] < a.gmin[d] || P[d] > a.gmax[d]) bad = 1;  // emulator.py:377-378
    }
    __syncthreads();
    double* __restrict__ kv = a.kbuf + (int64_t)b * mM;
    if (bad) {
        if (tid == 0 && a.info) a.info[b] = SF_INFO_OUT_OF_GRID;
        for (int e = tid; e < mM; e += 256) kv[e] = 0.0;  // keeps the batched product finite
        return;
    }
    // v12 blocks: kernels.py:25-26 (cdist of X/l and Z/l, sqeuclidean)
    for (int e = tid; e < mM; e += 256) {
        const int i = e / a.M, j = e - i * a.M;
        double d2 = 0.0;
        for (int d = 0; d < a.P; ++d) {
            const double l = a.lengthscales[i * a.P + d];
            const double df = a.grid[j * a.P + d] / l - P[d] / l;
            d2 = d2 + df * df;
        }
        kv[e] = a.variances[i] * exp(-0.5 * d2);
    }
    __syncthreads();
    for (int i = 0; i < a.m; ++i) {
        double acc = 0.0;
        for (int j = tid; j < a.M; j += 256) acc += kv[i * a.M + j] * a.alpha[i * a.M + j];
        acc = sf_block_sum(acc, red);
        if (tid == 0) a.mu[(int64_t)b * a.m + i] = acc;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_emu_z(sf_emu_args a, int B) {
    extern __shared__ double ksm[];  // EMU_WCHUNK x M: k_i of this chunk's walkers
    const int mM = a.m * a.M;
    const int i = blockIdx.y, b0 = blockIdx.z * EMU_WCHUNK;
    const int r = blockIdx.x * 256 + threadIdx.x;
    for (int e = threadIdx.x; e < EMU_WCHUNK * a.M; e += 256) {
        const int w = e / a.M, j = e - w * a.M;
        ksm[e] = (b0 + w < B) ? a.kbuf[(int64_t)(b0 + w) * mM + i * a.M + j] : 0.0;
    }
    __syncthreads();
    if (r >= mM) return;
    double acc[EMU_WCHUNK];
#pragma unroll
    for (int w = 0; w < EMU_WCHUNK; ++w) acc[w] = 0.0;
    // columns beyond r are zero in Linv (lower triangular): j <= r - i M
    const int jmax = min(a.M, r - i * a.M + 1);
    const double* __restrict__ lt = a.LinvT + (int64_t)i * a.M * mM + r;  // LinvT[c][r] = Linv[r][c]
    for (int j = 0; j < jmax; ++j) {
        const double l = lt[(int64_t)j * mM];
#pragma unroll
        for (int w = 0; w < EMU_WCHUNK; ++w) acc[w] += l * ksm[w * a.M + j];
    }
#pragma unroll
    for (int w = 0; w < EMU_WCHUNK; ++w)
        if (b0 + w < B) a.zscratch[((int64_t)(b0 + w) * mM + r) * a.m + i] = acc[w];
}

__global__ __launch_bounds__(256) void k_emu_post(sf_emu_args a) {
    extern __shared__ double esm[];
    double* covs = esm;  // m x m
    const int b = blockIdx.x, tid = threadIdx.x;
    if (a.info && a.info[b] != 0) return;
    const int mM = a.m * a.M;
    const double* __restrict__ z = a.zscratch + (int64_t)b * mM * a.m;
    // z^T z over the m M rows: every thread takes rows tid, tid + 256, ... and keeps a chunk of up to EMU_PAIRS
    // (i, j <= i) partial sums in registers; waves fold with shuffles, the four wave sums meet in LDS (fixed order)
    constexpr int EMU_PAIRS = 36;
    __shared__ double wsum[4][EMU_PAIRS];
    const int npairs = a.m * (a.m + 1) / 2;
    for (int p0 = 0; p0 < npairs; p0 += EMU_PAIRS) {
        const int np = min(EMU_PAIRS, npairs - p0);
        double acc[EMU_PAIRS];
#pragma unroll
        for (int q = 0; q < EMU_PAIRS; ++q) acc[q] = 0.0;
        // first pair of the chunk -> (i0, j0), row-major over the lower triangle
        int i0 = 0;
        while ((i0 + 1) * (i0 + 2) / 2 <= p0) ++i0;
        const int j0 = p0 - i0 * (i0 + 1) / 2;
        for (int r = tid; r < mM; r += 256) {
            const double* zr = z + (int64_t)r * a.m;
            int i = i0, j = j0;
#pragma unroll
            for (int q = 0; q < EMU_PAIRS; ++q) {
                if (q < np) {
                    acc[q] += zr[i] * zr[j];
                    if (++j > i) {
                        ++i;
                        j = 0;
                    }
                }
            }
        }
#pragma unroll
        for (int q = 0; q < EMU_PAIRS; ++q) {
            const double v = sf_wave_sum(acc[q]);
            if ((tid & 63) == 0) wsum[tid >> 6][q] = v;
        }
        __syncthreads();
        if (tid < np) {
            int i = i0, j = j0;
            for (int q = 0; q < tid; ++q)
                if (++j > i) {
                    ++i;
                    j = 0;
                }
            const double tot = wsum[0][tid] + wsum[1][tid] + wsum[2][tid] + wsum[3][tid];
            const double v = ((i == j) ? a.variances[i] : 0.0) - tot;  // v22 is diag(variances) at a single point
            covs[i * a.m + j] = v;
            covs[j * a.m + i] = v;
        }
        __syncthreads();
    }
    if (a.cov)
        for (int e = tid; e < a.m * a.m; e += 256) a.cov[(int64_t)b * a.m * a.m + e] = covs[e];
    __syncthreads();
    if (a.Lw) {
        // small dense Cholesky of Sigma_w (spectrum_model.py:334 cho_factor(weights_cov)): factor in LDS (in
        // place in `covs`, lower triangle), one thread, then a parallel copy-out with the upper part zeroed
        __shared__ int fail;
        if (tid == 0) {
            fail = 0;
            const int m = a.m;
            for (int j = 0; j < m; ++j) {
                double d = covs[j * m + j];
                for (int k = 0; k < j; ++k) d -= covs[j * m + k] * covs[j * m + k];
                if (!(d > 0.0)) { fail = 1; d = 1.0; }
                const double dj = sqrt(d), rj = 1.0 / dj;
                covs[j * m + j] = dj;
                for (int i = j + 1; i < m; ++i) {
                    double v = covs[i * m + j];
                    for (int k = 0; k < j; ++k) v -= covs[i * m + k] * covs[j * m + k];
                    covs[i * m + j] = v * rj;
                }
            }
            if (fail && a.info) a.info[b] = SF_INFO_BAD_WEIGHT_COV;
        }
        __syncthreads();
        double* L = a.Lw + (int64_t)b * a.m * a.m;
        for (int e = tid; e < a.m * a.m; e += 256) {
            const int i = e / a.m, j = e - i * a.m;
            L[e] = j <= i ? covs[e] : 0.0;
        }
    }
}

int sf_launch_emulator(const sf_emu_args& a, int B, hipStream_t s) {
    const size_t shm_z = sizeof(double) * (size_t)EMU_WCHUNK * a.M;
    if (shm_z > 64 * 1024 || a.m > SF_MAX_M) {
        sf_set_error("emulator: M=%d / m=%d too large", a.M, a.m);
        return SF_EINVAL;
    }
    if (!a.kbuf) {
        sf_set_error("emulator: the v12 scratch is missing");
        return SF_EINVAL;
    }
    const int mM = a.m * a.M;
    hipLaunchKernelGGL(k_emu_prep, dim3(B), dim3(256), 0, s, a);
    SF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_emu_z, dim3((mM + 255) / 256, a.m, (B + EMU_WCHUNK - 1) / EMU_WCHUNK), dim3(256), shm_z, s, a, B);
    SF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_emu_post, dim3(B), dim3(256), sizeof(double) * (size_t)a.m * a.m, s, a);
    SF_LAUNCH_CHECK();
    return SF_OK;
}

// Joint GP conditional over B query points (Emulator.__call__ with several parameter rows,
// emulator.py:382-389): with z_b = Linv v12_b left in zscratch by k_emu_z,
//   cov[(i,a),(j,b)] = delta_ij var_i exp(-1/2 |(p_a - p_b)/l_i|^2) - z_a[:, i] . z_b[:, j],
// indices component-major (i*B + a) as produced by the reference's block-diagonal batch_kernel.
__global__ __launch_bounds__(256) void k_emu_joint(sf_emu_args a, int B, const double* __restrict__ mu_pts,
                                                   double* __restrict__ mu, double* __restrict__ cov) {
    const int n = a.m * B, mM = a.m * a.M;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n) {
        const int i = (int)(e / B), pa = (int)(e - (int64_t)i * B);
        mu[e] = mu_pts[pa * a.m + i];
    }
    if (e >= (int64_t)n * n) return;
    const int I = (int)(e / n), J = (int)(e - (int64_t)I * n);
    const int i = I / B, pa = I - i * B, j = J / B, pb = J - j * B;
    const double* za = a.zscratch + (int64_t)pa * mM * a.m + i;
    const double* zb = a.zscratch + (int64_t)pb * mM * a.m + j;
    double acc = 0.0;
    for (int r = 0; r < mM; ++r) acc += za[(int64_t)r * a.m] * zb[(int64_t)r * a.m];
    double v22 = 0.0;
    if (i == j) {
        const double* Pa = a.params + (int64_t)pa * a.pstride + a.off_grid;
        const double* Pb = a.params + (int64_t)pb * a.pstride + a.off_grid;
        double d2 = 0.0;
        for (int d = 0; d < a.P; ++d) {
            const double l = a.lengthscales[i * a.P + d];
            const double df = Pa[d] / l - Pb[d] / l;
            d2 += df * df;
        }
        v22 = a.variances[i] * exp(-0.5 * d2);
    }
    cov[e] = v22 - acc;
}

int sf_launch_emu_joint(const sf_emu_args& a, int B, const double* mu_pts, double* mu, double* cov, hipStream_t s) {
    const int64_t n = (int64_t)a.m * B, total = n * n;
    hipLaunchKernelGGL(k_emu_joint, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a, B, mu_pts, mu, cov);
    SF_LAUNCH_CHECK();
    return SF_OK;
}

// d_lnl = -(logdet + sqmah)/2, -inf where info != 0   (spectrum_model.py:405)
__global__ void k_finish(int B, const double* __restrict__ logdet, const double* __restrict__ sqmah,
                         const int* __restrict__ info, const int* __restrict__ info2,
                         double* __restrict__ lnl, int* __restrict__ info_out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int code = info ? info[b] : 0;
    if (code == 0 && info2) code = info2[b];
    double v = -(logdet[b] + sqmah[b]) / 2;
    if (code == 0 && !(v == v)) code = SF_INFO_NAN;
    if (code != 0) v = -INFINITY;
    lnl[b] = v;
    if (info_out) info_out[b] = code;
}

int sf_launch_finish(int B, const double* logdet, const double* sqmah, const int* info, const int* info2,
                     double* lnl, int* info_out, hipStream_t s) {
    hipLaunchKernelGGL(k_finish, dim3((B + 255) / 256), dim3(256), 0, s, B, logdet, sqmah, info, info2, lnl,
                       info_out);
    SF_LAUNCH_CHECK();
    return SF_OK;
}
