// Applying the factor to right-hand sides: L Z, L^-1 B, L^-T B and L^-T L^-1 B (the reference's cho_solve,
// Starfish/models/spectrum_model.py:404) for the L that the factorisation leaves: row-major, lower, true diagonal.  The
// strict upper triangle holds leftovers of C or partial tiles and is never read, inside the diagonal blocks either.
//
// One workgroup (4 waves) owns one (matrix, group of up to 16 right-hand sides) and sweeps the 64-row blocks of L; nothing
// is shared between workgroups and nothing waits but __syncthreads().  Per block: the off-diagonal part is a product on
// v_mfma_f64_16x16x4_f64 (wave w: 16 of the 64 rows of a row block, or 16 of the 64 columns of a column block, against the
// 16 right-hand sides), the 64 x 64 diagonal block is applied in LDS with one lane per row as k_trsv_logdet does.  The
// solution vectors do not fit the LDS (n x 16 doubles): they live in the output array, whose earlier blocks every block
// step reads back (same workgroup, same CU: ordered by the barrier).  Both sweeps are left-looking, so each reads L once:
// the forward sweep by row blocks (contiguous rows), the back sweep by column blocks (512-byte row segments).
// L Z has no chain: out of place it runs one workgroup per row block; in place one workgroup walks the row blocks from the
// last to the first, which overwrites only entries no later block reads.
#pragma once
#include "sf_device.h"

#define SF_AP_NR 16   // right-hand sides of a group: the N of the MFMA
#define SF_AP_LDV 68  // doubles between two right-hand sides of a 64-row block in LDS

struct sf_apply_args {
    const double* L;
    int n, lda;
    int64_t stride;
    const double* rhs;  // right-hand side r of matrix b: rhs + b * rhs_stride + r * ldr, n contiguous rows
    int ldr;
    int64_t rhs_stride;  // 0: one block shared by every matrix
    double* out;         // may be rhs (rhs_stride != 0, same strides)
    int ldo;
    int64_t out_stride;
    int nrhs, op, ngroups, row_blocks;  // row_blocks: workgroups per (matrix, group): n / 64 for L Z out of place, else 1
};

// sum over k in [k0, k1) of L[row][k] X[k][col]: lane (lq, l15) holds row l15 of the wave's 16 rows as the A operand and
// right-hand side l15 as the B operand, both at k = 16 t + 4 lq + j (any order of k sums the same products).  Lrow: row
// l15 of the wave; xcol: right-hand side l15 (read only where `has`).  Result: register r = (row lq + 4 r, right-hand side l15).
__device__ __forceinline__ sf_d4 sf_ap_sweep_rows(const double* Lrow, bool al_l, const double* xcol, bool al_x, bool has,
                                                  int k0, int k1, int lq) {
    sf_d4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int k = k0 + 4 * lq; k < k1; k += 16) {
        double a[4], x[4] = {0.0, 0.0, 0.0, 0.0};
        sf_ap_ld4(Lrow + k, al_l, a);
        if (has) sf_ap_ld4(xcol + k, al_x, x);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[j], x[j], acc, 0, 0, 0);
    }
    return acc;
}
// sum over rows r in [r0, r1) of L[r][col] X[r][rhs]: the transposed product of the back sweep.  Lcol: &L[0][column l15 of
// the wave's 16 columns].  Result: register r = (column lq + 4 r, right-hand side l15).
__device__ __forceinline__ sf_d4 sf_ap_sweep_cols(const double* Lcol, int lda, const double* xcol, bool al_x, bool has,
                                                  int r0, int r1, int lq) {
    sf_d4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int r = r0 + 4 * lq; r < r1; r += 16) {
        double a[4], x[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = Lcol[(int64_t)(r + j) * lda];
        if (has) sf_ap_ld4(xcol + r, al_x, x);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[j], x[j], acc, 0, 0, 0);
    }
    return acc;
}

// the lower triangle of the diagonal block at (c, c) -> Ts (64 x 65); zeros above the diagonal, which is not read from L
__device__ __forceinline__ void sf_ap_load_diag(const double* Mx, int lda, int c, double* Ts, int tid) {
    for (int e = tid; e < SF_LEAF * SF_LEAF; e += 256) {
        const int i = e >> 6, j = e & 63;
        Ts[i * 65 + j] = j <= i ? Mx[(int64_t)(c + i) * lda + c + j] : 0.0;
    }
}

// One block step of a substitution sweep.  FWD: X[c] = L_cc^-1 (B[c] - L[c, 0:c] X[0:c]); else X[c] = L_cc^-T (B[c] -
// L[c+64:n, c]^T X[c+64:n]).  B = src (ld lds), X = dst (ld ldd): src may be dst.  Ends with a barrier: X[c] is visible to
// the whole workgroup.
template <bool FWD>
__device__ __forceinline__ void sf_ap_solve_block(const double* Mx, int n, int lda, bool al_l, const double* src, int lds,
                                                  double* dst, int ldd, bool al_x, int nr, int c, double* Ts, double* Sv) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, lq = lane >> 4;
    sf_ap_load_diag(Mx, lda, c, Ts, tid);
    const bool has = l15 < nr;
    const double* xcol = dst + (int64_t)l15 * ldd;
    sf_d4 acc;
    if (FWD)
        acc = sf_ap_sweep_rows(Mx + (int64_t)(c + w * 16 + l15) * lda, al_l, xcol, al_x, has, 0, c, lq);
    else
        acc = sf_ap_sweep_cols(Mx + c + w * 16 + l15, lda, xcol, al_x, has, c + SF_LEAF, n, lq);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = w * 16 + lq + 4 * r;
        Sv[l15 * SF_AP_LDV + i] = (has ? src[(int64_t)l15 * lds + c + i] : 0.0) - acc[r];
    }
    __syncthreads();
    // wave w: right-hand sides 4 w .. 4 w + 3, lane = row of the block
    double t[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) t[q] = Sv[(4 * w + q) * SF_AP_LDV + lane];
    if (FWD) {
#pragma unroll 4
        for (int k = 0; k < SF_LEAF; ++k) {
            const double d = Ts[k * 65 + k], lk = Ts[lane * 65 + k];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double zk = __shfl(t[q], k) / d;
                t[q] = lane > k ? t[q] - lk * zk : (lane == k ? zk : t[q]);
            }
        }
    } else {
#pragma unroll 4
        for (int k = SF_LEAF - 1; k >= 0; --k) {
            const double d = Ts[k * 65 + k], lk = lane < k ? Ts[k * 65 + lane] : 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double zk = __shfl(t[q], k) / d;
                t[q] = lane < k ? t[q] - lk * zk : (lane == k ? zk : t[q]);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (4 * w + q < nr) dst[(int64_t)(4 * w + q) * ldd + c + lane] = t[q];
    __syncthreads();
}

// Y[c] = L[c, 0:c] Z[0:c] + L_cc Z[c].  Z = src, Y = dst (may be src: the caller walks the blocks downwards).
__device__ __forceinline__ void sf_ap_multiply_block(const double* Mx, int lda, bool al_l, const double* src, int lds,
                                                     bool al_s, double* dst, int ldd, int nr, int c, double* Ts,
                                                     double* Sv, double* Zs) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, lq = lane >> 4;
    sf_ap_load_diag(Mx, lda, c, Ts, tid);
    const bool has = l15 < nr;
    const sf_d4 acc = sf_ap_sweep_rows(Mx + (int64_t)(c + w * 16 + l15) * lda, al_l, src + (int64_t)l15 * lds, al_s, has, 0,
                                       c, lq);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = w * 16 + lq + 4 * r;
        Sv[l15 * SF_AP_LDV + i] = acc[r];
        Zs[l15 * SF_AP_LDV + i] = has ? src[(int64_t)l15 * lds + c + i] : 0.0;
    }
    __syncthreads();
    double y[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) y[q] = Sv[(4 * w + q) * SF_AP_LDV + lane];
#pragma unroll 4
    for (int k = 0; k < SF_LEAF; ++k) {
        const double lk = Ts[lane * 65 + k];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double zk = Zs[(4 * w + q) * SF_AP_LDV + k];
            if (k <= lane) y[q] = __builtin_fma(lk, zk, y[q]);
        }
    }
    __syncthreads();  // every read of Z[c] is done: Y[c] may land on it
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (4 * w + q < nr) dst[(int64_t)(4 * w + q) * ldd + c + lane] = y[q];
}

__global__ __launch_bounds__(256) void k_chol_apply(const sf_apply_args a) {
    __shared__ __attribute__((aligned(16))) double Ts[SF_LEAF * 65];
    __shared__ __attribute__((aligned(16))) double Sv[SF_AP_NR * SF_AP_LDV];
    __shared__ __attribute__((aligned(16))) double Zs[SF_AP_NR * SF_AP_LDV];
    const int bid = blockIdx.x;
    const int rb = bid % a.row_blocks, g = (bid / a.row_blocks) % a.ngroups, b = bid / (a.row_blocks * a.ngroups);
    const int nr = min(SF_AP_NR, a.nrhs - g * SF_AP_NR), nb = a.n / SF_LEAF;
    const double* Mx = a.L + (int64_t)b * a.stride;
    const double* src = a.rhs + (int64_t)b * a.rhs_stride + (int64_t)g * SF_AP_NR * a.ldr;
    double* dst = a.out + (int64_t)b * a.out_stride + (int64_t)g * SF_AP_NR * a.ldo;
    // 16-byte loads where the rows allow them (uniform over the workgroup)
    const bool al_l = (((uintptr_t)Mx & 15) | (a.lda & 1)) == 0;
    const bool al_s = (((uintptr_t)src & 15) | (a.ldr & 1)) == 0;
    const bool al_d = (((uintptr_t)dst & 15) | (a.ldo & 1)) == 0;
    if (a.op == SF_APPLY_L) {
        for (int cb = nb - 1 - rb; cb >= 0; cb -= a.row_blocks)
            sf_ap_multiply_block(Mx, a.lda, al_l, src, a.ldr, al_s, dst, a.ldo, nr, cb * SF_LEAF, Ts, Sv, Zs);
        return;
    }
    if (a.op != SF_APPLY_LINVT) {
        for (int cb = 0; cb < nb; ++cb)
            sf_ap_solve_block<true>(Mx, a.n, a.lda, al_l, src, a.ldr, dst, a.ldo, al_d, nr, cb * SF_LEAF, Ts, Sv);
        if (a.op == SF_APPLY_LINV) return;
        src = dst;  // C^-1: the back sweep goes over the forward sweep's result in place
    }
    const int lds = a.op == SF_APPLY_LINVT ? a.ldr : a.ldo;
    for (int cb = nb - 1; cb >= 0; --cb)
        sf_ap_solve_block<false>(Mx, a.n, a.lda, al_l, src, lds, dst, a.ldo, al_d, nr, cb * SF_LEAF, Ts, Sv);
}

int sf_launch_chol_apply(const double* L, int n, int lda, int64_t stride, int batch, int op, const double* rhs, int nrhs,
                         int ldr, int64_t rhs_stride, double* out, int ldo, int64_t out_stride, hipStream_t s) {
    sf_apply_args a;
    a.L = L, a.n = n, a.lda = lda, a.stride = stride;
    a.rhs = rhs, a.ldr = ldr, a.rhs_stride = rhs_stride;
    a.out = out, a.ldo = ldo, a.out_stride = out_stride;
    a.nrhs = nrhs, a.op = op;
    a.ngroups = (nrhs + SF_AP_NR - 1) / SF_AP_NR;
    a.row_blocks = (op == SF_APPLY_L && (const double*)out != rhs) ? n / SF_LEAF : 1;
    const long long grid = (long long)batch * a.ngroups * a.row_blocks;
    if (grid > 0x7fffffffLL) {
        sf_set_error("chol_apply: %lld workgroups exceed one launch", grid);
        return SF_EINVAL;
    }
    hipLaunchKernelGGL(k_chol_apply, dim3((unsigned)grid), dim3(256), 0, s, a);
    SF_LAUNCH_CHECK();
    return SF_OK;
}

// ---- the context-level call: staging of the right-hand sides in the workspace and export of the results
// stage[b][r][0:npad) = rhs of (b, r) on the n data rows (rhs NULL: the walker's own residual, nrhs = 1), zero on the padding
__global__ void k_apply_stage(const double* __restrict__ rhs, int ldr, int64_t rhs_stride, const double* __restrict__ resid,
                              int n, int npad, int nrhs, double* __restrict__ stage) {
    const int r = blockIdx.y, b = blockIdx.z;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npad) return;
    double v = 0.0;
    if (i < n) v = rhs ? rhs[(int64_t)b * rhs_stride + (int64_t)r * ldr + i] : resid[(int64_t)b * npad + i];
    stage[((int64_t)b * nrhs + r) * npad + i] = v;
}
// out[b][r][0:n) = the data rows of stage, NaN for the walkers whose status is not 0
__global__ void k_apply_export(const double* __restrict__ stage, const int* __restrict__ info, int n, int npad, int nrhs,
                               double* __restrict__ out) {
    const int r = blockIdx.y, b = blockIdx.z;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double v = stage[((int64_t)b * nrhs + r) * npad + i];
    out[((int64_t)b * nrhs + r) * n + i] = info[b] != 0 ? __builtin_nan("") : v;
}
int sf_launch_apply_stage(const double* rhs, int ldr, int64_t rhs_stride, const double* resid, int n, int npad, int nrhs,
                          int batch, double* stage, hipStream_t s) {
    hipLaunchKernelGGL(k_apply_stage, dim3((npad + 255) / 256, nrhs, batch), dim3(256), 0, s, rhs, ldr, rhs_stride, resid, n,
                       npad, nrhs, stage);
    SF_LAUNCH_CHECK();
    return SF_OK;
}
int sf_launch_apply_export(const double* stage, const int* info, int n, int npad, int nrhs, int batch, double* out,
                           hipStream_t s) {
    hipLaunchKernelGGL(k_apply_export, dim3((n + 255) / 256, nrhs, batch), dim3(256), 0, s, stage, info, n, npad, nrhs, out);
    SF_LAUNCH_CHECK();
    return SF_OK;
}
