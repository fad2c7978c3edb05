// The full banded solve x = A^-1 rhs: the keeping forward sweep, the backward sweep, and the Woodbury mix that turns
// T = Bd^-1 [r, Y^T] into [alpha, V] = C^-1 [r, X^T] for the mean-flux gradient.
//
//   forward   k_band_keep<NRB>: k_band_forms' sweep (sf_band_sweep_body.h with SFB_SWEEP_KEEP), which besides logdet and the Gram matrix
//             stores per block column F_k = L_kk^-1, the blocks L_{k+1+I,k} and W_k = (L^-1 rhs)_k  (sfb_keep_block)
//   backward  k_band_back<NRB>: T_k^T = ( W_k^T - sum_I T_{k+1+I}^T L_{k+1+I,k} ) F_k, block columns from the last to the first
//   mix       k_band_mix_matrix: M from the Gram matrix and Lw;  k_band_mix: stage = T M per pixel (any number of leading
//             right-hand sides in front of Y: the gradient's one residual, the diagnostics' k)
#pragma once
#include "sf_band_sweep.h"

#define SFB_SWEEP_KERNEL k_band_keep
#define SFB_SWEEP_KEEP 1
#include "sf_band_sweep_body.h"
#undef SFB_SWEEP_KERNEL
#undef SFB_SWEEP_KEEP

// Single (untwisted) window sweep that keeps the factor in fac: sfb_keep_doubles(c.n, nbr, nrb) doubles per matrix
int sf_launch_band_keep(const sf_band_call& c, double* fac, hipStream_t s) {
    const int nrhs = c.r.nrhs;
    if (c.n <= 0 || c.batch <= 0 || c.halfwidth < 0 || c.ldb < c.halfwidth + 1 || !fac || sfb_admit(c.halfwidth, nrhs) != SFB_WINDOW) {
        sf_set_error("band_keep: bad arguments, or the half-width exceeds the LDS window (n=%d halfwidth=%d ldb=%d nrhs=%d)", c.n,
                     c.halfwidth, c.ldb, nrhs);
        return SF_EINVAL;
    }
    sf_band_args a = band_args(c);
    a.logdet = c.logdet, a.gram = c.gram;
    a.nhalf = 1;
    const int nbr = a.nbr, nrb = sfb_nrb(nrhs), nwaves = sfb_nwaves(nbr);
    const sf_band_keep kp = {fac, (int64_t)sfb_keep_doubles(c.n, nbr, nrb)};
    const size_t shm = sfb_lds_layout(nbr, nrb).bytes;
    static sf_dev_once attr_once;
    SF_CHECK(sf_lds_limit_once(&attr_once, SFB_LDS_MAX,
                               {(const void*)k_band_keep<1>, (const void*)k_band_keep<2>, (const void*)k_band_keep<3>}));
    if (sfb_loader_groups(nwaves) * SFB_PF < nbr || nwaves * 64 < (nbr - 1 + nrb) * BB) {
        sf_set_error("band_keep: window too large for one workgroup");
        return SF_EINVAL;
    }
    const dim3 blk(nwaves * 64);
    if (nrb == 1) hipLaunchKernelGGL(k_band_keep<1>, dim3(c.batch), blk, shm, s, a, kp);
    else if (nrb == 2) hipLaunchKernelGGL(k_band_keep<2>, dim3(c.batch), blk, shm, s, a, kp);
    else hipLaunchKernelGGL(k_band_keep<3>, dim3(c.batch), blk, shm, s, a, kp);
    SF_LAUNCH_CHECK();
    return SF_OK;
}

// Backward sweep, one workgroup per matrix, SFB_BACK_SPLIT waves per block of 16 right-hand sides.  The solved blocks T_j^T
// (rows = right-hand sides, columns = pixels) of the last nbr - 1 columns live in an LDS ring; the factor's block column
// comes from global memory straight into MFMA operand registers (lane (l15, lq) of product kk holds L[4 lq + kk][l15]: 16
// lanes read 128 contiguous bytes), and column k - 1 is requested before this step's products are issued.  Per step k:
//   wave (rb, s)   acc = (s == 0 ? W_k^T : 0) - sum_{I = s, s + 4, ..} T_{k+1+I}^T L_{k+1+I,k}   -> part[rb][s]
//   barrier
//   wave (rb, 0)   T_k^T = (part[rb][0] + part[rb][1] + part[rb][2] + part[rb][3]) F_k   -> ring slot k % nbr, and x
//   barrier
// Every sum has one order, whatever the batch.  A matrix with info != 0 gets NaN and nothing of it is read.
struct sf_band_back_args {
    const double* fac;  // the keeping sweep's records
    int64_t sfac;
    const int* info;    // [batch]
    double* x;          // x[b * sx + r * ldx + i], r < nrhs, i < n
    int64_t sx;
    int ldx, n, nbr, nrhs;
};
template <int NRB>
__global__ __launch_bounds__(64 * SFB_BACK_SPLIT * NRB) void k_band_back(sf_band_back_args a) {
    extern __shared__ double lds[];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rb = wave / SFB_BACK_SPLIT, sp = wave % SFB_BACK_SPLIT;
    const int l15 = lane & 15, lq = lane >> 4;
    const int n = a.n, nbr = a.nbr, nb1 = nbr - 1, nblk = (n + BB - 1) / BB;
    double* x = a.x + (int64_t)b * a.sx;
    if (a.info[b] != 0) {
        for (int r = 0; r < a.nrhs; ++r)
            for (int i = tid; i < n; i += blockDim.x) x[(int64_t)r * a.ldx + i] = __builtin_nan("");
        return;
    }
    const sfb_back_lds L = sfb_back_lds_layout(nbr, NRB);
    double* Tr = lds + L.T + rb * nbr * BS;                        // this wave's ring
    double* part = lds + L.part + rb * SFB_BACK_SPLIT * BS;        // the partial sums of its block of right-hand sides
    const double* fac = a.fac + (int64_t)b * a.sfac;
    const int oAB = l15 * BLD + 4 * lq;                            // A operand: row l15, K slice 4 lq .. 4 lq + 3
    const int oB = 4 * lq * BB + l15;                              // B operand from a stored block: rows 4 lq + kk, column l15
    const int oD = lq * BB + l15;                                  // accumulator rows lq + 4 r of a stored block

    // operands of one step: this wave's factor blocks, and for the wave with sp == 0 the right-hand sides and F_k
    sf_d4 Lr[SFB_BACK_MAX_BLOCKS], Fr, Wr;
    auto request = [&](int k) {
        const int cnt = min(nb1, nblk - 1 - k);
#pragma unroll
        for (int q = 0; q < SFB_BACK_MAX_BLOCKS; ++q) {
            const int I = sp + q * SFB_BACK_SPLIT;
            if (I < cnt) {
                const double* Lb = fac + sfb_keep_block(k, 1 + I, nbr, NRB) + oB;
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) Lr[q][kk] = Lb[kk * BB];
            }
        }
        if (sp == 0) {
            const double* Fb = fac + sfb_keep_block(k, 0, nbr, NRB) + oB;
            const double* Wb = fac + sfb_keep_block(k, nbr + rb, nbr, NRB) + oD;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) Fr[kk] = Fb[kk * BB], Wr[kk] = Wb[4 * kk * BB];
        }
    };
    request(nblk - 1);
    int ks = (nblk - 1) % nbr;
    for (int k = nblk - 1; k >= 0; --k, ks = ks == 0 ? nbr - 1 : ks - 1) {
        const int cnt = min(nb1, nblk - 1 - k);
        sf_d4 acc = {0.0, 0.0, 0.0, 0.0};
        if (sp == 0) acc = Wr;
        sf_d4 av[SFB_BACK_MAX_BLOCKS];
#pragma unroll
        for (int q = 0; q < SFB_BACK_MAX_BLOCKS; ++q) {
            const int I = sp + q * SFB_BACK_SPLIT;
            if (I < cnt) {
                int slot = ks + 1 + I;
                slot = slot >= nbr ? slot - nbr : slot;
                const double* Ap = Tr + slot * BS + oAB;
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) av[q][kk] = Ap[kk];
            }
        }
#pragma unroll
        for (int q = 0; q < SFB_BACK_MAX_BLOCKS; ++q)
            if (sp + q * SFB_BACK_SPLIT < cnt) {
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[q][kk], Lr[q][kk], acc, 0, 0, 1);  // neg: -A B + C
            }
        const sf_d4 Fk = Fr;
        if (k > 0) request(k - 1);  // lands under the rest of this step
#pragma unroll
        for (int r = 0; r < 4; ++r) part[sp * BS + (lq + 4 * r) * BLD + l15] = acc[r];
        __syncthreads();
        if (sp == 0) {
            sf_d4 t = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                double s = part[oAB + kk];
#pragma unroll
                for (int w = 1; w < SFB_BACK_SPLIT; ++w) s += part[w * BS + oAB + kk];
                t = __builtin_amdgcn_mfma_f64_16x16x4f64(s, Fk[kk], t, 0, 0, 0);
            }
            const int col = k * BB + l15;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = rb * BB + lq + 4 * r;
                Tr[ks * BS + (lq + 4 * r) * BLD + l15] = t[r];
                if (row < a.nrhs && col < n) x[(int64_t)row * a.ldx + col] = t[r];
            }
        }
        __syncthreads();
    }
}

int sf_launch_band_back(const double* fac, int n, int halfwidth, int batch, int nrhs, const int* info, double* x, int ldx, int64_t sx,
                        hipStream_t s) {
    if (!fac || !info || !x || n <= 0 || batch <= 0 || ldx < n || sfb_admit(halfwidth, nrhs) != SFB_WINDOW) {
        sf_set_error("band_back: bad arguments, or the half-width exceeds the LDS window (n=%d halfwidth=%d nrhs=%d ldx=%d)", n, halfwidth,
                     nrhs, ldx);
        return SF_EINVAL;
    }
    const int nbr = sfb_nbr(halfwidth), nrb = sfb_nrb(nrhs);
    if (sfb_back_blocks_per_wave(nbr) > SFB_BACK_MAX_BLOCKS) {
        sf_set_error("band_back: window too large for one workgroup");
        return SF_EINVAL;
    }
    const size_t shm = sfb_back_lds_layout(nbr, nrb).bytes;
    static sf_dev_once attr_once;
    SF_CHECK(sf_lds_limit_once(&attr_once, SFB_LDS_MAX,
                               {(const void*)k_band_back<1>, (const void*)k_band_back<2>, (const void*)k_band_back<3>}));
    const sf_band_back_args a = {fac, (int64_t)sfb_keep_doubles(n, nbr, nrb), info, x, sx, ldx, n, nbr, nrhs};
    const dim3 blk(64 * sfb_back_nwaves(nrb));
    if (nrb == 1) hipLaunchKernelGGL(k_band_back<1>, dim3(batch), blk, shm, s, a);
    else if (nrb == 2) hipLaunchKernelGGL(k_band_back<2>, dim3(batch), blk, shm, s, a);
    else hipLaunchKernelGGL(k_band_back<3>, dim3(batch), blk, shm, s, a);
    SF_LAUNCH_CHECK();
    return SF_OK;
}

// The mix matrix of the Woodbury identity, one wave per walker, for kr leading right-hand sides R in front of the m rows of Y
// (the sweep's rows are [R; Y], nin = kr + m of them; the gradient's [r; Y] is kr = 1).  With g_c = gram[kr:, c],
// G = gram[kr:, kr:], S = I + G = L_S L_S^T:
//   alpha_c = t_c - T_Y S^-1 g_c  (c < kr),   V = C^-1 X^T = T_Y S^-1 Lw^T      (X^T = Y^T Lw^T; nv = m columns, or nv = 0: none)
// so [alpha, V] = T M with the nin x nout matrix M, nout = kr + nv: M[r][c] = (r == c) for r < kr, M[kr + j][c] = -(S^-1 g_c)_j
// for c < kr, M[kr + j][kr + k] = (S^-1 Lw^T)_jk.  Lane c solves column c of S Z = [g_0 .. g_{kr-1}, Lw^T].  A walker with
// info != 0 is not read.  flag (may be NULL; the walkers' status, where k_woodbury has not looked at S): a non-positive pivot
// of S sets SF_INFO_BAD_WEIGHT_COV there.
#define SFB_MIX_MAX SFB_MIX_MAX_ROWS  // rows and columns of M: what three blocks of right-hand sides hold
#define SFB_MIX_LD 49
__global__ __launch_bounds__(64) void k_band_mix_matrix(const double* __restrict__ gram, const double* __restrict__ Lw, int kr, int m,
                                                        int nv, const int* info, int* flag, double* __restrict__ M) {
    __shared__ double S[33 * 33];
    __shared__ double Z[32 * SFB_MIX_LD];  // Z[j * SFB_MIX_LD + c]
    const int b = blockIdx.x, lane = threadIdx.x, nin = kr + m, nout = kr + nv;
    if (info[b] != 0) return;
    const double* g = gram + (int64_t)b * nin * nin;
    const double* lw = Lw + (int64_t)b * m * m;
    for (int e = lane; e < m * m; e += 64) {
        const int r = e / m, c = e - r * m;
        S[r * 33 + c] = g[(r + kr) * nin + (c + kr)] + (r == c ? 1.0 : 0.0);
    }
    for (int e = lane; e < m * nout; e += 64) {
        const int j = e / nout, c = e - j * nout;
        Z[j * SFB_MIX_LD + c] = c < kr ? g[(j + kr) * nin + c] : (j <= c - kr ? lw[(c - kr) * m + j] : 0.0);  // Lw^T[j][c - kr]
    }
    __syncthreads();
    int bad = 0;
    for (int j = 0; j < m; ++j) {  // S = L_S L_S^T in place (lower), as k_woodbury
        const double p = S[j * 33 + j];
        if (!(p > 0.0)) bad = 1;
        const double rs = 1.0 / sqrt(p);
        __syncthreads();
        double lij = 0.0;
        if (lane > j && lane < m) {
            lij = S[lane * 33 + j] * rs;
            S[lane * 33 + j] = lij;
        }
        if (lane == j) S[j * 33 + j] = rs;  // (the diagonal holds 1 / l_jj)
        __syncthreads();
        if (lane > j && lane < m)
            for (int c = j + 1; c <= lane; ++c) S[lane * 33 + c] -= lij * S[c * 33 + j];
        __syncthreads();
    }
    if (lane < nout) {
        const int c = lane;
        for (int j = 0; j < m; ++j) {  // L_S z = rhs
            double v = Z[j * SFB_MIX_LD + c];
            for (int i = 0; i < j; ++i) v -= S[j * 33 + i] * Z[i * SFB_MIX_LD + c];
            Z[j * SFB_MIX_LD + c] = v * S[j * 33 + j];
        }
        for (int j = m - 1; j >= 0; --j) {  // L_S^T y = z
            double v = Z[j * SFB_MIX_LD + c];
            for (int i = j + 1; i < m; ++i) v -= S[i * 33 + j] * Z[i * SFB_MIX_LD + c];
            Z[j * SFB_MIX_LD + c] = v * S[j * 33 + j];
        }
        double* Mb = M + (int64_t)b * nin * nout;
        for (int r = 0; r < kr; ++r) Mb[r * nout + c] = r == c ? 1.0 : 0.0;
        for (int j = 0; j < m; ++j) Mb[(kr + j) * nout + c] = c < kr ? -Z[j * SFB_MIX_LD + c] : Z[j * SFB_MIX_LD + c];
    }
    if (flag && bad && lane == 0) flag[b] = SF_INFO_BAD_WEIGHT_COV;  // (info[b] was 0)
}
// stage[b][c][i] = (c < nself ? T[b][c][i] M[b][c][c] : 0) + sum_{j >= lead} T[b][j][i] M[b][j][c], j ascending, for the nin rows
// of T and the nin x nout matrix M (the rows j < lead of a column hold its own unit entry or zeros: they are not multiplied
// out); pixels n .. npad - 1 are zero.  One thread per pixel.
__global__ __launch_bounds__(256) void k_band_mix(const double* __restrict__ T, const double* __restrict__ M, const int* __restrict__ info,
                                                  int nin, int lead, int nself, int nout, int n, int npad, double* __restrict__ stage) {
    __shared__ double Ms[SFB_MIX_MAX * SFB_MIX_MAX];
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (info[b] != 0) return;
    for (int e = threadIdx.x; e < nin * nout; e += 256) Ms[e] = M[(int64_t)b * nin * nout + e];
    __syncthreads();
    if (i >= npad) return;
    const double* Tb = T + (int64_t)b * nin * npad;
    double* sb = stage + (int64_t)b * nout * npad;
    for (int c = 0; c < nout; ++c) {
        double v = 0.0;
        if (i < n) {
            if (c < nself) v += Tb[(int64_t)c * npad + i] * Ms[c * nout + c];
            for (int j = lead; j < nin; ++j) v += Tb[(int64_t)j * npad + i] * Ms[j * nout + c];
        }
        sb[(int64_t)c * npad + i] = v;
    }
}
// gram: [batch][(kr + m)^2] of the sweep over [R; Y]; Lw: [batch][m][m] (not read with nv = 0); T: [batch][kr + m][npad] of the
// backward sweep; Mwork: [batch][(kr + m)(kr + nv)]; stage: [batch][kr + nv][npad]; flag: see k_band_mix_matrix
int sf_launch_band_mix(const double* gram, const double* Lw, int kr, int m, int nv, const int* info, int* flag, const double* T, int n,
                       int npad, int batch, double* Mwork, double* stage, hipStream_t s) {
    if (m < 1 || m > 32 || kr < 1 || kr + m > SFB_MIX_MAX || (nv != 0 && nv != m) || kr + nv > SFB_MIX_MAX || batch <= 0 ||
        batch > 65535 || n <= 0 || npad < n) {
        sf_set_error("band_mix: 1 .. 32 low-rank rows, at most %d rows of right-hand sides in all, 1 .. 65535 walkers", SFB_MIX_MAX);
        return SF_EINVAL;
    }
    hipLaunchKernelGGL(k_band_mix_matrix, dim3(batch), dim3(64), 0, s, gram, Lw, kr, m, nv, info, flag, Mwork);
    SF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_band_mix, dim3((npad + 255) / 256, batch), dim3(256), 0, s, T, Mwork, info, kr + m, kr, kr, kr + nv, n, npad,
                       stage);
    SF_LAUNCH_CHECK();
    return SF_OK;
}
