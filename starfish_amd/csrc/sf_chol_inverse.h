// The diagonal of C^-1 = L^-T L^-1 from the factor: d_j = sum over i >= j of (L^-1)_ij^2, the squared norm of column j of
// X = L^-1, for the L that the factorisation leaves (row-major, lower, true diagonal, order a multiple of 64; nothing above
// the diagonal is read before this layer has written it).  With d and alpha = C^-1 r the leave-one-out predictive of pixel i
// is r_i - alpha_i / d_i with variance 1 / d_i (Rasmussen & Williams, Gaussian Processes for Machine Learning, 5.4.2).
//
// In column blocks of 64:  X_JJ = L_JJ^-1,  X_IJ = -L_II^-1 sum_{K=J}^{I-1} L_IK X_KJ  for I > J.
//   k_chol_block_inverse  one workgroup per (matrix, diagonal block): L_II^-1 by forward substitution in LDS, one lane per
//                         row, stored TRANSPOSED in the workspace, winv[matrix][I][column][row].
//   k_chol_inverse_diag   one workgroup (4 waves) owns one (matrix, column block J) from start to end; column blocks are
//                         independent, so nothing waits but __syncthreads(), there are no atomics, and every sum has a fixed
//                         order (a repeated call gives the same bits).  Per row block I the long sum is a 64 x 64 tile on
//                         v_mfma_f64_16x16x4_f64 (wave w: rows 16 w .. 16 w + 15 of the tile against its 64 columns: four
//                         accumulators), then the product with winv[I] (the tile goes through LDS to become the B operand).
// Where X lives: X_IJ (I > J) is stored transposed in the strict upper triangle of the matrix, row block J, columns 64 I ..,
// which is dead after the factorisation: column c of the block column is row 64 J + c of the matrix, contiguous in the row
// index of X -- the "right-hand side r, n contiguous rows" layout that sf_ap_ld4 reads as an MFMA operand.  The segments of
// two workgroups are disjoint and lie outside the diagonal blocks; X_JJ is read from winv.  The lower triangle is never
// written.  L is read n^3 / 384 doubles per matrix (64-wide blocks), X as often.
// Identity padding: rows of L that are rows of the identity give X_ij = 0 exactly for a data column j, so the padding adds
// nothing to d_j.
#pragma once
#include "sf_chol_apply.h"

#define SF_INV_LDS 68  // row stride of the S tile in LDS ([k][column]: the B operand's 16 lanes x 4 quarters hit distinct banks)
#define SF_INV_LDX 65  // row stride of the X tile in LDS ([column][row]: rows out coalesced, columns summed without conflicts)

struct sf_inverse_args {
    double* L;
    int n, lda;
    int64_t stride;
    double* winv;  // [batch][n / 64][64][64]: (L_II^-1)^T
    double* out;   // d of matrix b: out + b * out_stride, n entries
    int64_t out_stride;
    int nb, batch;
};

__global__ __launch_bounds__(256) void k_chol_block_inverse(const sf_inverse_args a) {
    __shared__ double Ts[SF_LEAF * 65];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int I = blockIdx.x % a.nb, b = blockIdx.x / a.nb;
    sf_ap_load_diag(a.L + (int64_t)b * a.stride, a.lda, I * SF_LEAF, Ts, tid);
    __syncthreads();
    // wave w: columns 16 w .. 16 w + 15 of the inverse, lane = row; column c is zero above row c, so k starts at 16 w
    const double rdiag = 1.0 / Ts[lane * 65 + lane];
    double t[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) t[q] = lane == 16 * w + q ? 1.0 : 0.0;
#pragma unroll 2
    for (int k = 16 * w; k < SF_LEAF; ++k) {
        const double rd = __shfl(rdiag, k), lk = Ts[lane * 65 + k];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const double zk = __shfl(t[q], k) * rd;
            t[q] = lane > k ? __builtin_fma(-lk, zk, t[q]) : (lane == k ? zk : t[q]);
        }
    }
    double* W = a.winv + ((int64_t)b * a.nb + I) * (SF_LEAF * SF_LEAF);
#pragma unroll
    for (int q = 0; q < 16; ++q) W[(16 * w + q) * SF_LEAF + lane] = t[q];
}

// dacc += the squares of rows 16 sq .. 16 sq + 15 of column sc of the X tile, in row order
__device__ __forceinline__ double sf_inv_squares(const double* Xs, int sc, int sq, double dacc) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const double v = Xs[sc * SF_INV_LDX + 16 * sq + r];
        dacc = __builtin_fma(v, v, dacc);
    }
    return dacc;
}

__global__ __launch_bounds__(256) void k_chol_inverse_diag(const sf_inverse_args a) {
    __shared__ __attribute__((aligned(16))) double Tile[SF_LEAF * SF_INV_LDS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, lq = lane >> 4;
    // the long column blocks (small J) start first; the workgroups of one matrix share an XCD when batch is a multiple of 8
    const int b = blockIdx.x % a.batch, J = blockIdx.x / a.batch, c0 = J * SF_LEAF;
    double* Mx = a.L + (int64_t)b * a.stride;
    const double* Wb = a.winv + (int64_t)b * a.nb * (SF_LEAF * SF_LEAF);
    const double* WJ = Wb + (int64_t)J * (SF_LEAF * SF_LEAF);
    const bool al_l = (((uintptr_t)Mx & 15) | (a.lda & 1)) == 0, al_w = ((uintptr_t)a.winv & 15) == 0;
    const int sc = tid & 63, sq = tid >> 6;  // column and row quarter whose squares this thread sums

    // X_JJ = L_JJ^-1: winv holds it as [column][row] already
    for (int e = tid; e < SF_LEAF * SF_LEAF; e += 256) Tile[(e >> 6) * SF_INV_LDX + (e & 63)] = WJ[e];
    __syncthreads();
    double dacc = sf_inv_squares(Tile, sc, sq, 0.0);
    __syncthreads();

    const double *xw[4], *xu[4];  // column 16 t + l15 of X indexed by the absolute k: in winv (K = J) and in the upper triangle
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        xw[t] = WJ + (16 * t + l15) * SF_LEAF - c0;
        xu[t] = Mx + (int64_t)(c0 + 16 * t + l15) * a.lda;
    }
    for (int I = J + 1; I < a.nb; ++I) {
        const int r0 = I * SF_LEAF;
        sf_d4 acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = sf_d4{0.0, 0.0, 0.0, 0.0};
        const double* Lrow = Mx + (int64_t)(r0 + 16 * w + l15) * a.lda;
        sf_inv_sweep(Lrow, al_l, xw, al_w, c0, c0 + SF_LEAF, lq, acc);
        sf_inv_sweep(Lrow, al_l, xu, al_l, c0 + SF_LEAF, r0, lq, acc);
        // S -> LDS as [k][column]; register r of acc[t] = (row 16 w + lq + 4 r, column 16 t + l15)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) Tile[(16 * w + lq + 4 * r) * SF_INV_LDS + 16 * t + l15] = acc[t][r];
        __syncthreads();
        // X_IJ = -L_II^-1 S: rows 16 w .. of a lower triangular factor need k < 16 (w + 1); (L_II^-1)[i][k] = winv[I][k][i]
        const double* WI = Wb + (int64_t)I * (SF_LEAF * SF_LEAF) + 16 * w + l15;
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = sf_d4{0.0, 0.0, 0.0, 0.0};
        for (int s = 0; s <= w; ++s) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = 16 * s + 4 * lq + j;
                const double li = WI[k * SF_LEAF];
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(li, Tile[k * SF_INV_LDS + 16 * t + l15], acc[t], 0, 0, 0);
            }
        }
        __syncthreads();  // every read of S is done: X may land on it, as [column][row]
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) Tile[(16 * t + l15) * SF_INV_LDX + 16 * w + lq + 4 * r] = -acc[t][r];
        __syncthreads();
        for (int e = tid; e < SF_LEAF * SF_LEAF; e += 256)
            Mx[(int64_t)(c0 + (e >> 6)) * a.lda + r0 + (e & 63)] = Tile[(e >> 6) * SF_INV_LDX + (e & 63)];
        dacc = sf_inv_squares(Tile, sc, sq, dacc);
        __syncthreads();  // X_IJ is visible to the next long sum (same workgroup), and the tile is free again
    }
    Tile[sq * SF_LEAF + sc] = dacc;
    __syncthreads();
    if (tid < SF_LEAF)
        a.out[(int64_t)b * a.out_stride + c0 + tid] =
            ((Tile[tid] + Tile[SF_LEAF + tid]) + Tile[2 * SF_LEAF + tid]) + Tile[3 * SF_LEAF + tid];
}

size_t sf_chol_inverse_work_doubles(int n, int batch) {
    if (n <= 0 || batch <= 0) return 0;
    return (size_t)batch * (size_t)(n / SF_LEAF) * (SF_LEAF * SF_LEAF);
}
int sf_launch_chol_inverse_diag(double* L, int n, int lda, int64_t stride, int batch, double* winv, double* out,
                                int64_t out_stride, hipStream_t s) {
    sf_inverse_args a;
    a.L = L, a.n = n, a.lda = lda, a.stride = stride;
    a.winv = winv, a.out = out, a.out_stride = out_stride;
    a.nb = n / SF_LEAF, a.batch = batch;
    const long long grid = (long long)batch * a.nb;
    if (grid > 0x7fffffffLL) {
        sf_set_error("chol_inverse_diag: %lld workgroups exceed one launch", grid);
        return SF_EINVAL;
    }
    hipLaunchKernelGGL(k_chol_block_inverse, dim3((unsigned)grid), dim3(256), 0, s, a);
    SF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_chol_inverse_diag, dim3((unsigned)grid), dim3(256), 0, s, a);
    SF_LAUNCH_CHECK();
    return SF_OK;
}

// diag[b][i] = A_b[i][i], i < n: the diagonal of what the factorisation is about to overwrite
__global__ void k_diag_copy(const double* __restrict__ A, int n, int lda, int64_t stride, double* __restrict__ diag) {
    const int b = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) diag[(int64_t)b * n + i] = A[(int64_t)b * stride + (int64_t)i * (lda + 1)];
}
int sf_launch_diag_copy(const double* A, int n, int lda, int64_t stride, int batch, double* diag, hipStream_t s) {
    hipLaunchKernelGGL(k_diag_copy, dim3((n + 255) / 256, batch), dim3(256), 0, s, A, n, lda, stride, diag);
    SF_LAUNCH_CHECK();
    return SF_OK;
}
