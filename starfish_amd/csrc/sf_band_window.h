// What the kernels of the band solver share: their arguments, the slot of a block in the window, the generic fetch of one
// window element and the read-out of the symmetric Gram accumulator.
#pragma once
#include "sf_common.h"
#include "sf_band_shape.h"
#include "sf_device.h"

struct sf_band_args {
    const double* band;  // [batch] x sband : band[i*ldb + d] = A[i][i-d], d in [0, halfwidth]
    int64_t sband;
    int ldb;
    int halfwidth;
    sf_band_rhs r;
    int n;      // matrix order
    int nbr;    // window blocks per side
    double* logdet;  // [batch]
    double* gram;    // [batch][nrhs*nrhs]
    int* info;       // [batch] first non-positive pivot (1-based), left untouched otherwise
    // optional additive terms of a final pass over a merged separator block (twisted factorisation)
    const double* logdet_add;  // [batch]
    const double* gram_add;    // [batch][nrhs*nrhs]
    int info_off;              // added to the reported pivot column (separator pass)
    // Two-sided ("twisted") sweep: grid = 2 * batch, workgroup 2b eliminates block columns [0, kend0)
    // top-down, workgroup 2b+1 eliminates the last kend1 block columns bottom-up (the same algorithm on
    // the index-reversed matrix); both stop at the nm-row separator and dump what is left of it.
    int nhalf;                 // 1 = ordinary single sweep
    int kend0, kend1;
    double* dumpM;             // [batch][2][nm*nm]   separator block, lower triangle, local row-major
    double* dumpR;             // [batch][2][NR*nm]   right-hand-side rows over the separator columns
    double* dumpG;             // [batch][2][nrhs*nrhs] partial Gram matrices
    double* dumpL;             // [batch][2]          partial log-determinants
};

// Where the keeping sweep (k_band_keep, sf_band_solve.h) stores what it eliminates: per block column one record of
// sfb_keep_column_blocks blocks (sfb_keep_block)
struct sf_band_keep {
    double* fac;   // [batch] x sfac
    int64_t sfac;
};

__device__ __forceinline__ int sfb_pair(int a, int b) {  // slot of the unordered pair {a, b}
    return a >= b ? a * (a + 1) / 2 + b : b * (b + 1) / 2 + a;
}

// Entry (r, c) of the Gram matrix from its accumulator G = -Z Z^T, of which only the lower triangle is maintained
__device__ __forceinline__ double sfb_gram(const double* G, int ldg, int r, int c) {
    return -((c <= r) ? G[r * ldg + c] : G[c * ldg + r]);
}

// One element of block row gb of one matrix for the initial window fill (generic, off the critical path).
// e < nbr*256: band blocks (gb, gb-nbr+1 .. gb) row-major inside each block; then NR*16 rhs entries.
// `rev` >= 0: the sweep runs on the index-reversed matrix, i -> rev - i (rev = padded order - 1).
// rhs, rhs0, nrhs, ldr: the matrix's sf_band_rhs, taken apart (passed as a struct it changes the sweep's instruction order).
__device__ __noinline__ double sfb_fetch(const double* band, const double* rhs, const double* rhs0, int gb,
                                         int e, int nbr, int n, int halfwidth, int ldb, int nrhs, int ldr,
                                         int rev) {
    const int row_elems = nbr * BB * BB;
    if (e < row_elems) {
        const int blk = e >> 8, r = (e >> 4) & 15, cc = e & 15;
        const int gc = gb - nbr + 1 + blk;
        const int i = gb * BB + r, d = i - (gc * BB + cc);
        if (gc < 0 || d < 0) return 0.0;
        const int io = rev >= 0 ? rev - i + d : i;  // larger original index of the pair
        if (io < n) return d <= halfwidth ? band[(int64_t)io * ldb + d] : 0.0;
        return d == 0 ? 1.0 : 0.0;  // identity padding up to a multiple of 16
    }
    const int q = e - row_elems, r = q >> 4, cc = q & 15;
    const int i = gb * BB + cc;
    const int io = rev >= 0 ? rev - i : i;
    if (io >= n || io < 0 || r >= nrhs) return 0.0;
    return sf_band_rhs{rhs, 0, ldr, nrhs, rhs0, 0}.row(r)[io];
}
