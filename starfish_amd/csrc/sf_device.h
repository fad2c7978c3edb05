// Device helpers shared by the .hip files: lane and wave primitives and the XCD remap of block ids (all four files), and
// the Cholesky of a 16 x 16 block in the MFMA accumulator layout (k_diag_mfma, sf_diag_lds_body; sf_band.hip keeps its own),
// and the k-contiguous operand reads of the 64-column MFMA sweep (the factor's application, its inverse, the gradient).
// Floating-point contraction: the helpers spell every fused multiply-add as __builtin_fma and hold no other candidate,
// so the objects built with -ffp-contract=off (sf_fill, sf_transform) and the others get the same code from them.
#pragma once
#include "sf_common.h"

__device__ __forceinline__ double sf_readlane_d(double v, int srclane) {
    union { double d; int i[2]; } u;
    u.d = v;
    u.i[0] = __builtin_amdgcn_readlane(u.i[0], srclane);
    u.i[1] = __builtin_amdgcn_readlane(u.i[1], srclane);
    return u.d;
}

// 1/sqrt(p): hardware estimate + two Newton steps (full double precision for p > 0)
__device__ __forceinline__ double sf_rsqrt(double p) {
    double y = __builtin_amdgcn_rsq(p);
    const double h = 0.5 * p;
    double e = __builtin_fma(-h * y, y, 0.5);
    y = __builtin_fma(y, e, y);
    e = __builtin_fma(-h * y, y, 0.5);
    y = __builtin_fma(y, e, y);
    return y;
}

// sum over the 64 lanes of a wave, in every lane
__device__ __forceinline__ double sf_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// Logical block id such that ids adjacent in work space run on the same XCD (block b is observed on
// XCD b % 8; each XCD has its own L2).  Bijective for any grid size; placement only affects speed.
__device__ __forceinline__ int sf_xcd_remap(int bid, int nblk) {
    const int xcd = bid & 7, slot = bid >> 3;
    const int q = nblk >> 3, r = nblk & 7;
    const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + slot;
}

// ---- operands of v_mfma_f64_16x16x4_f64 read k-contiguously (sf_chol_apply.h, sf_chol_inverse.h, sf_cinv.h)
// four consecutive doubles; al: p is 16-byte aligned
__device__ __forceinline__ void sf_ap_ld4(const double* p, bool al, double (&v)[4]) {
    if (al) {
        const double2 lo = *(const double2*)p, hi = *(const double2*)(p + 2);
        v[0] = lo.x, v[1] = lo.y, v[2] = hi.x, v[3] = hi.y;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = p[j];
    }
}

// acc[t] += sum over k in [k0, k1) of L[row][k] X[k][16 t + l15]: Lrow = row l15 of the wave's 16 rows, xc[t] = column
// 16 t + l15 of X indexed by k.  Lane (lq, l15) holds k = 16 s + 4 lq + j of both operands.
__device__ __forceinline__ void sf_inv_sweep(const double* Lrow, bool al_l, const double* (&xc)[4], bool al_x, int k0,
                                             int k1, int lq, sf_d4 (&acc)[4]) {
    if (k0 >= k1) return;
    // the operands of the next 16 columns are read under this step's products (the last step reads its own again)
    double l[4], x[4][4];
    sf_ap_ld4(Lrow + k0 + 4 * lq, al_l, l);
#pragma unroll
    for (int t = 0; t < 4; ++t) sf_ap_ld4(xc[t] + k0 + 4 * lq, al_x, x[t]);
    for (int kk = k0; kk < k1; kk += 16) {
        const int kn = min(kk + 16, k1 - 16) + 4 * lq;
        double ln[4], xn[4][4];
        sf_ap_ld4(Lrow + kn, al_l, ln);
#pragma unroll
        for (int t = 0; t < 4; ++t) sf_ap_ld4(xc[t] + kn, al_x, xn[t]);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(l[j], x[t][j], acc[t], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            l[j] = ln[j];
#pragma unroll
            for (int t = 0; t < 4; ++t) x[t][j] = xn[t][j];
        }
    }
}

// One wave: Cholesky of the symmetric 16 x 16 block a0 AND the inverse of its factor, both kept in the MFMA
// accumulator layout (lane (lq, l15) = (lane >> 4, lane & 15), register r <-> element (lq + 4r, l15)).  Column j of the
// symmetric block is also its row j = register j/4 of the 16 lanes of quarter j%4, which is exactly where a K-slice of
// the MFMA operands lives: the rank-1 elimination  A -= v v^T  and the update of F = L^-1 (F -= v g^T) are one
// v_mfma_f64_16x16x4_f64 each, with no data movement at all.  The next pivot a_{j+1,j+1} - l_{j+1,j}^2 comes from
// scalars, so that its rsqrt chain runs while the matrix core applies this column's rank-1 update.
// a0 (sf_d4 variable, consumed), lane, l15, lq: of the caller.  Outputs, variables the caller declares: sf_d4 f = L^-1,
// sf_d4 lt = L^T (lt[r] of lane (lq, l15) = L[l15][lq + 4r], zero above the diagonal of L) and double pkeep = pivot j
// before its square root in lane j < 16 (1.0 in the other lanes): the caller derives the non-positive-pivot report from
// it.  One statement; its locals (r, j, p, rs, v, g, ...) stay inside, so no argument may carry one of their names.
// A macro, not a function: the kernels that use it sit at their register limits, and a callee that the compiler
// simplifies on its own before it inlines it comes out in another instruction order (k_diag_mfma: 108 -> 128 VGPRs
// and spills; k_diag_lds and k_potrf_dataflow changed too).  As text the step compiles to the code it had in place.
#define SF_POTRF16_ACC(a0, lane, l15, lq, f, lt, pkeep)                                                           \
    do {                                                                                                          \
        _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                           \
            f[r] = ((lq) + 4 * r) == (l15) ? 1.0 : 0.0;                                                           \
            lt[r] = 0.0;                                                                                          \
        }                                                                                                         \
        double p = sf_readlane_d((a0)[0], 0);                                                                     \
        pkeep = 1.0;                                                                                              \
        _Pragma("unroll") for (int j = 0; j < 16; ++j) {                                                          \
            const int qj = j & 3, rj = j >> 2;                                                                    \
            pkeep = (lane) == j ? p : pkeep;                                                                      \
            const double rs = sf_rsqrt(p);                                                                        \
            const bool in_q = (lq) == qj;                                                                         \
            const double v = (in_q && (l15) > j) ? (a0)[rj] * rs : 0.0; /* l_ij, i = l15 > j */                   \
            const double g = in_q ? f[rj] * rs : 0.0;                 /* row j of F, scaled */                    \
            if (in_q) {                                                                                           \
                f[rj] = g;                                                                                        \
                lt[rj] = (l15) == j ? p * rs : v; /* L^T[j][i] */                                                 \
            }                                                                                                     \
            if (j + 1 < 16) {                                                                                     \
                const double an = sf_readlane_d((a0)[(j + 1) >> 2], ((j + 1) & 3) * 16 + j + 1);                  \
                const double vn = sf_readlane_d(v, qj * 16 + j + 1);                                              \
                p = __builtin_fma(-vn, vn, an);                                                                   \
            }                                                                                                     \
            (a0) = __builtin_amdgcn_mfma_f64_16x16x4f64(v, v, (a0), 0, 0, 1); /* blgp = neg:[1,0,0]: -A B + C */  \
            f = __builtin_amdgcn_mfma_f64_16x16x4f64(v, g, f, 0, 0, 1);                                           \
        }                                                                                                         \
    } while (0)
