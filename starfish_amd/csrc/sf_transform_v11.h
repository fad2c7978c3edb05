// Emulator training: the covariance v11 of the training likelihood built on the device, one matrix (k_v11_build) or a
// batch of hyper-parameter rows in one launch (k_v11_build_batch).   Starfish/emulator/emulator.py:126-128,569-571
#pragma once
#include "sf_device.h"
#include "sf_transform.h"

// ---------------------------------------------------------------------------------------------
// v11 = iPhiPhi / lambda_xi + blockdiag_c( variance_c exp(-1/2 |(x_i - x_j) / lengthscale_c|^2) )  of the emulator's
// training likelihood (Starfish/emulator/emulator.py:126-128,569-571; kernels.py:5-49), built ON the device into the
// padded layout the batched Cholesky takes (identity block from n = m M to npad): Emulator.train evaluates it once per
// objective call, and the host build + upload of the 1320 x 1320 matrix of the worked example cost 5x the
// factorisation.  hyper = [lambda_xi, variances[m], lengthscales[m][P]] (device).  Operation order of the reference:
// (x / l) differences squared and summed over the parameters in order, -0.5 * d2, exp, times the variance, added to
// iPhiPhi / lambda_xi.
__global__ __launch_bounds__(256) void k_v11_build(const double* __restrict__ grid, int M, int P, int m,
                                                   const double* __restrict__ hyper, const double* __restrict__ iphiphi,
                                                   double* __restrict__ A, int npad, int lda) {
    const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (j >= npad) return;
    const int n = m * M;
    double v;
    if (i < n && j < n) {
        v = iphiphi[(int64_t)i * n + j] / hyper[0];
        const int ci = i / M, cj = j / M;
        if (ci == cj) {
            const double* gi = grid + (int64_t)(i - ci * M) * P;
            const double* gj = grid + (int64_t)(j - cj * M) * P;
            const double* ls = hyper + 1 + m + ci * P;
            double d2 = 0.0;
            for (int p = 0; p < P; ++p) {
                const double d = gi[p] / ls[p] - gj[p] / ls[p];
                d2 = d2 + d * d;
            }
            v = v + hyper[1 + ci] * exp(-0.5 * d2);
        }
    } else {
        v = (i == j) ? 1.0 : 0.0;
    }
    A[(int64_t)i * lda + j] = v;
}
int sf_launch_v11_build(const double* grid, int M, int P, int m, const double* hyper, const double* iphiphi, double* A, int npad,
                        int lda, hipStream_t s) {
    if (!grid || !hyper || !iphiphi || !A || M <= 0 || P <= 0 || m <= 0 || npad < m * M || lda < npad) {
        sf_set_error("v11_build: bad arguments");
        return SF_EINVAL;
    }
    hipLaunchKernelGGL(k_v11_build, dim3((npad + 255) / 256, npad), dim3(256), 0, s, grid, M, P, m, hyper, iphiphi, A, npad, lda);
    SF_LAUNCH_CHECK();
    return SF_OK;
}

// ---------------------------------------------------------------------------------------------
// The same matrix for B hyper-parameter rows (hyper + b * hyper_stride, RAW values as above) in ONE launch: what
// Emulator.train needs when a simplex iteration is evaluated as one batch (sf_emulator_loglike_batch).  Matrix b goes to
// A + b * stride in the padded layout of sf_potrf_batch; columns npad..lda of a row are never touched.
// One workgroup owns a 64 x 64 tile of one matrix; with lower_only the tiles strictly above the diagonal return at once
// (entries above the diagonal inside a diagonal tile are written: the contract of sf_cov_fill_batch).  What a tile costs
// is decided per WORKGROUP:
//   - wholly in the padding: identity / zero, nothing read;
//   - its row and column ranges meet no common component: iPhiPhi / lambda_xi alone (per element, with the identity
//     where the tile reaches past n);
//   - otherwise the RBF term: the scaled coordinates grid[r][p] / ls[c(r)][p] of its 64 rows and 64 columns are staged in
//     LDS first -- 128 P divisions per tile where k_v11_build does 2 P per ELEMENT -- and the sum over p runs on their
//     differences in the reference's order.  A tile inside one component adds it to every element; one that straddles
//     a component boundary or n tests ci == cj per element as k_v11_build does (a row's scaled coordinates use the
//     lengthscales of the row's own component, so wherever ci == cj the operands are k_v11_build's).
// Each thread owns two adjacent columns of eight rows and writes them as 16-byte stores (lda, stride and the tile origin
// are even); a wave covers two full 512-byte tile rows per store.  The diagonal tiles also write the replicated
// right-hand side R[b][0..npad) = w_hat, 0, ... the solve reads.
// Rate: NOT measured.  A write-bound kernel by construction (8 bytes stored per element against one fp64 division, one
// exp and P multiply-adds); it is to be priced against sf_debug_stream_write like the covariance fill.
#define SF_V11_T 64
#define SF_V11_PMAX 8
__global__ __launch_bounds__(256) void k_v11_build_batch(const double* __restrict__ grid, int M, int P, int m,
                                                         const double* __restrict__ hyper, int hyper_stride,
                                                         const double* __restrict__ iphiphi, double* __restrict__ A, int npad,
                                                         int lda, int64_t stride, int lower_only,
                                                         const double* __restrict__ w_hat, double* __restrict__ R, int ldr) {
    const int tj = blockIdx.x, ti = blockIdx.y, b = blockIdx.z;
    if (lower_only && tj > ti) return;
    __shared__ __attribute__((aligned(16))) double xr[SF_V11_PMAX][SF_V11_T];  // scaled coordinates of the tile's rows
    __shared__ __attribute__((aligned(16))) double xc[SF_V11_PMAX][SF_V11_T];  // ... and of its columns
    __shared__ double vr[SF_V11_T];                                            // variance of each row's component
    __shared__ int cr[SF_V11_T], cc[SF_V11_T];                                 // component of each row / column, -1: padding
    const int n = m * M, i0 = ti * SF_V11_T, j0 = tj * SF_V11_T, tid = threadIdx.x;
    const double* hb = hyper + (int64_t)b * hyper_stride;
    double* Ab = A + (int64_t)b * stride;
    if (R && ti == tj && tid < SF_V11_T) R[(int64_t)b * ldr + i0 + tid] = i0 + tid < n ? w_hat[i0 + tid] : 0.0;
    const int cx = (tid & 31) * 2, ry = tid >> 5;  // this thread: columns j0 + cx, + 1 of rows i0 + ry + 8 k
    if (i0 >= n || j0 >= n) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int i = i0 + ry + 8 * k, j = j0 + cx;
            *(double2*)(Ab + (int64_t)i * lda + j) = make_double2(i == j ? 1.0 : 0.0, i == j + 1 ? 1.0 : 0.0);
        }
        return;
    }
    const int ci0 = i0 / M, ci1 = min(i0 + SF_V11_T - 1, n - 1) / M, cj0 = j0 / M, cj1 = min(j0 + SF_V11_T - 1, n - 1) / M;
    const bool rbf = ci0 <= cj1 && cj0 <= ci1;  // the component ranges of rows and columns meet
    const bool whole = ci0 == ci1 && cj0 == cj1 && ci0 == cj0 && i0 + SF_V11_T <= n && j0 + SF_V11_T <= n;
    if (rbf) {
        if (tid < 2 * SF_V11_T) {
            const int side = tid >> 6, r = tid & 63, g = (side ? j0 : i0) + r;
            double* x = side ? &xc[0][r] : &xr[0][r];
            int c = -1;
            if (g < n) {
                c = g / M;
                const double* gp = grid + (int64_t)(g - c * M) * P;
                const double* ls = hb + 1 + m + c * P;
                for (int p = 0; p < P; ++p) x[p * SF_V11_T] = gp[p] / ls[p];
            } else {
                for (int p = 0; p < P; ++p) x[p * SF_V11_T] = 0.0;
            }
            (side ? cc : cr)[r] = c;
            if (!side) vr[r] = c >= 0 ? hb[1 + c] : 0.0;
        }
        __syncthreads();
    }
    double d2[8][2];
#pragma unroll
    for (int k = 0; k < 8; ++k) d2[k][0] = d2[k][1] = 0.0;
    if (rbf) {
        for (int p = 0; p < P; ++p) {
            const double2 c2 = *(const double2*)&xc[p][cx];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const double xi = xr[p][ry + 8 * k];
                const double da = xi - c2.x, db = xi - c2.y;
                d2[k][0] = d2[k][0] + da * da;
                d2[k][1] = d2[k][1] + db * db;
            }
        }
    }
    const double lam = hb[0];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int r = ry + 8 * k, i = i0 + r;
        double v[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int j = j0 + cx + e;
            if (whole || (i < n && j < n)) {
                v[e] = iphiphi[(int64_t)i * n + j] / lam;
                if (whole || (rbf && cr[r] == cc[cx + e])) v[e] = v[e] + vr[r] * exp(-0.5 * d2[k][e]);
            } else {
                v[e] = (i == j) ? 1.0 : 0.0;
            }
        }
        *(double2*)(Ab + (int64_t)i * lda + j0 + cx) = make_double2(v[0], v[1]);
    }
}
int sf_launch_v11_build_batch(const double* grid, int M, int P, int m, const double* hyper, int hyper_stride, int B,
                              const double* iphiphi, double* A, int npad, int lda, int64_t stride, int lower_only,
                              const double* w_hat, double* R, int ldr, hipStream_t s) {
    if (!grid || !hyper || !iphiphi || !A || M <= 0 || P <= 0 || m <= 0 || B <= 0 || B > 65535) {
        sf_set_error("v11_build_batch: bad arguments");
        return SF_EINVAL;
    }
    if (P > SF_V11_PMAX) {
        sf_set_error("v11_build_batch: P=%d grid dimensions, at most %d (the tile's scaled coordinates live in LDS)", P, SF_V11_PMAX);
        return SF_EINVAL;
    }
    if ((int64_t)m * M > npad || npad % SF_V11_T != 0 || npad / SF_V11_T > 65535 || lda < npad ||
        stride < (int64_t)(npad - 1) * lda + npad || (int64_t)hyper_stride < 1 + (int64_t)m + (int64_t)m * P) {
        sf_set_error("v11_build_batch: npad (a multiple of %d) >= m M, lda >= npad, stride >= one matrix and hyper_stride >= "
                     "1 + m + m P are required", SF_V11_T);
        return SF_EINVAL;
    }
    // the 16-byte stores
    if ((lda & 1) || (stride & 1) || ((uintptr_t)A & 15)) {
        sf_set_error("v11_build_batch: lda and stride must be even and d_A 16-byte aligned");
        return SF_EINVAL;
    }
    if (R && (!w_hat || ldr < npad)) {
        sf_set_error("v11_build_batch: the right-hand side needs w_hat and ldr >= npad");
        return SF_EINVAL;
    }
    const int nt = npad / SF_V11_T;
    hipLaunchKernelGGL(k_v11_build_batch, dim3(nt, nt, B), dim3(256), 0, s, grid, M, P, m, hyper, hyper_stride, iphiphi, A, npad,
                       lda, stride, lower_only, w_hat, R, ldr);
    SF_LAUNCH_CHECK();
    return SF_OK;
}
