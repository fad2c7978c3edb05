// Blocks of C^-1 = X^T X, X = L^-1, from what sf_launch_chol_inverse_diag leaves: X_KJ (K > J) transposed in the strict upper
// triangle (row 64 J + c, columns 64 K ..), X_JJ transposed in winv[J], zero above its diagonal.  A layer of sf_fill.hip; the
// gradient layers (sf_grad_frame.h) contract these tiles.
//
//   sf_cinv_tile     G_IJ = sum_{K >= I} X_KI^T X_KJ for J <= I on v_mfma_f64_16x16x4_f64: both operands are k-contiguous
//                    (sf_inv_sweep).  Four waves; wave w holds rows 16 w .. 16 w + 15 of block I against the 64 columns of
//                    block J in four accumulators, register r of acc[t] = (row 16 w + lq + 4 r, column 16 t + l15).
//   k_cinv_blocks    one workgroup per (matrix, listed pair): the tile, stored (sf_potri_blocks_batch).
// Nothing of the lower triangle is written.
#pragma once

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
