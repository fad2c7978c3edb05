// What the likelihood gradients of sf_cov_grad.h and sf_emu_grad.h share (Rasmussen & Williams, Gaussian Processes for Machine
// Learning, eq. 5.9):
//     d lnL / d theta = 1/2 sum_ij (alpha_i alpha_j - (C^-1)_ij) (dC / d theta)_ij,   alpha = C^-1 r
// contracted block row by block row from the 64 x 64 tiles of C^-1 (sf_cinv.h).  A layer of sf_fill.hip.  A contraction kernel
// is one 4-wave workgroup per (matrix, block row I), short I first (their K sums are the long ones), matrix fastest; it walks
// the pairs J <= I it needs in ascending order and per pair
//   sf_grad_tile     forms the tile and A_ij = alpha_i alpha_j - G_ij for i, j < n, zero beyond (the rows: sf_grad_rows);
//   (its own part)   multiplies A with the derivative entries of one slot at a time and sums per thread over (t, r);
//   sf_grad_put      sums over the wave (xor shuffles) and leaves the wave's sum in LDS;
//   sf_grad_flush    has thread 0 add the four waves' sums, in wave order, times the pair's weight (sf_grad_weight: 2 for
//                    J < I, 1 for J == I, where the whole tile is formed), to the slot's running sum in LDS.
// Partial sums per (matrix, block row, slot) go to the workspace (sf_grad_part), and
//   k_grad_sum       one thread per (matrix, slot) adds the block rows in ascending order, times 1/2; NaN where info != 0.
//   k_multi_grad_reduce  the sum over the orders of a multi-order gradient, per (walker, column), in ascending order index.
// No atomics, no workgroup waits for another, every sum in a fixed order (a repeated call gives the same bits); nothing of
// the lower triangle is written; rows and columns >= n are not read as data (their alpha and entries are masked) and
// nothing is written for them.
#pragma once

// the output side of a contraction, embedded in its argument struct
struct sf_grad_out {
    const int* info;  // [batch]: != 0 -> NaN rows, nothing is read
    double* part;     // [batch][nbr][nslots]: sf_grad_part_doubles
    int nbr, nslots, batch;
    double* grad;     // [batch][grad_stride]
    int grad_stride;
};
static inline size_t sf_grad_part_doubles(size_t n, int nslots, int batch) {
    return (size_t)batch * ((n + SF_LEAF - 1) / SF_LEAF) * (size_t)nslots;
}

// block index -> (matrix, block row); false for a matrix that failed: k_grad_sum writes NaN and does not read its partial sums
__device__ __forceinline__ bool sf_grad_block(const sf_grad_out& o, int& b, int& I) {
    b = blockIdx.x % o.batch, I = blockIdx.x / o.batch;
    return o.info[b] == 0;
}
__device__ __forceinline__ double* sf_grad_part(const sf_grad_out& o, int b, int I) {
    return o.part + ((int64_t)b * o.nbr + I) * o.nslots;
}
// this thread's rows 16 w + lq + 4 r of the block row that starts at R0: alpha, masked beyond n
__device__ __forceinline__ void sf_grad_rows(const double* al, int R0, int n, int w, int lq, double (&a_r)[4], bool (&ok_r)[4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = R0 + 16 * w + lq + 4 * r;
        ok_r[r] = i < n;
        a_r[r] = ok_r[r] ? al[i] : 0.0;
    }
}
// the weight of pair (I, J <= I) in the sum over the lower triangle: the whole tile is formed on the diagonal
__device__ __forceinline__ double sf_grad_weight(int I, int J) { return J < I ? 2.0 : 1.0; }
// The tile of pair (I, J) as A_ij = alpha_i alpha_j - G_ij, zero where a row or a column is beyond n; ok_c[t]: this thread's
// column 64 J + 16 t + l15 is below n
__device__ __forceinline__ void sf_grad_tile(const sf_cinv_src& src, const double* al, int n, int I, int J, int w, int l15, int lq,
                                             const double (&a_r)[4], const bool (&ok_r)[4], sf_d4 (&A)[4], bool (&ok_c)[4]) {
    sf_cinv_tile(src, I, J, w, l15, lq, A);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int j = J * SF_LEAF + 16 * t + l15;
        ok_c[t] = j < n;
        const double a_c = ok_c[t] ? al[j] : 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) A[t][r] = ok_r[r] && ok_c[t] ? a_r[r] * a_c - A[t][r] : 0.0;
    }
}
// a thread's sum over its entries -> the wave's, left at *red by lane 0
__device__ __forceinline__ void sf_grad_put(double v, double* red, int lane) {
    v = sf_wave_sum(v);
    if (lane == 0) *red = v;
}
// red[w * stride + q] holds wave w's sum of value q < nv: thread 0 adds the four in wave order, times wgt, to dst[q].  The
// first barrier publishes whatever the caller wrote to LDS before, the second one frees red.
__device__ __forceinline__ void sf_grad_flush(int nv, double wgt, const double* red, int stride, double* dst, int tid) {
    __syncthreads();
    if (tid == 0)
        for (int q = 0; q < nv; ++q)
            dst[q] = dst[q] + wgt * (((red[q] + red[stride + q]) + red[2 * stride + q]) + red[3 * stride + q]);
    __syncthreads();
}

__global__ void k_grad_sum(const sf_grad_out o) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (q >= o.nslots) return;
    double s = 0.0;
    if (o.info[b] != 0) {
        s = __builtin_nan("");
    } else {
        for (int I = 0; I < o.nbr; ++I) s = s + o.part[((int64_t)b * o.nbr + I) * o.nslots + q];
        s = 0.5 * s;
    }
    o.grad[(int64_t)b * o.grad_stride + q] = s;
}
// The sum over the orders of a multi-order gradient (sf_multi_grad_reduce): per-unit results stored order-major
// (unit = i * W + w), one thread per (walker, column).  Column j < ncols adds the unit slots its CSR list names, ascending in
// the segment: s = g0; s = s + g1; ... (0.0 without a source); column ncols is the walker's lnl, the same fixed-order sum over
// all the orders, and its status, the first non-zero unit code in ascending order.  A walker with a non-zero status gets
// lnl = -inf and NaN in every column.  A source outside the unit rows is not read: the column comes out NaN.
__global__ void k_multi_grad_reduce(const sf_multi_reduce_args a) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x, w = blockIdx.y;
    if (j > a.ncols) return;
    int code = 0;
    for (int i = 0; i < a.nseg && code == 0; ++i) code = a.unit_info[(int64_t)i * a.W + w];
    if (j == a.ncols) {
        double s = a.unit_lnl[w];
        for (int i = 1; i < a.nseg; ++i) s = s + a.unit_lnl[(int64_t)i * a.W + w];
        a.lnl[w] = code != 0 ? -__builtin_inf() : s;
        a.info[w] = code;
        return;
    }
    double s = 0.0;
    if (code != 0) {
        s = __builtin_nan("");
    } else {
        const int lo = a.col_ptr[j], hi = a.col_ptr[j + 1];
        for (int q = lo; q < hi; ++q) {
            const int i = a.col_src[2 * q], slot = a.col_src[2 * q + 1];
            double g = __builtin_nan("");
            if (i >= 0 && i < a.nseg && slot >= 0 && slot < a.grad_stride)
                g = a.unit_grad[((int64_t)i * a.W + w) * a.grad_stride + slot];
            s = q == lo ? g : s + g;
        }
    }
    a.grad[(int64_t)w * a.out_stride + j] = s;
}
int sf_launch_multi_grad_reduce(const sf_multi_reduce_args& a, hipStream_t s) {
    if (a.nseg < 1 || a.W < 1 || a.W > 65535 || a.ncols < 0 || a.grad_stride < 1 || a.out_stride < a.ncols) {
        sf_set_error("sf_multi_grad_reduce: nseg >= 1, W in 1 .. 65535, ncols >= 0, grad_stride >= 1 and out_stride >= ncols");
        return SF_EINVAL;
    }
    hipLaunchKernelGGL(k_multi_grad_reduce, dim3((a.ncols + 1 + 63) / 64, a.W), dim3(64), 0, s, a);
    SF_LAUNCH_CHECK();
    return SF_OK;
}

// the launch tail of a contraction: its block-row kernel over (matrix, block row), then the sum over the block rows
template <class Args>
static int sf_launch_grad(void (*kernel)(const Args), const Args& a, const sf_grad_out& o, hipStream_t s) {
    const long long grid = (long long)o.batch * o.nbr;
    SF_CHECK(sf_check_fill_grid(grid));
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(256), 0, s, a);
    SF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_grad_sum, dim3((o.nslots + 63) / 64, o.batch), dim3(64), 0, s, o);
    SF_LAUNCH_CHECK();
    return SF_OK;
}
