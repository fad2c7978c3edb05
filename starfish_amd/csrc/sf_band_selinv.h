// Selected inversion on the band: the entries of Sigma = A^-1 inside the band, from the factor the keeping sweep stores
// (k_band_keep, sf_band_solve.h), by Takahashi's recurrence over block columns from the last to the first.  With
// G_I = L_{k+1+I,k} F_k (F_k = L_kk^-1) and cnt = min(nbr - 1, nblk - 1 - k):
//   Sigma_{k+1+J,k} = - sum_{I < cnt} Sigma_{k+1+J,k+1+I} G_I         (J < cnt;  Sigma_{a,b} = Sigma_{b,a}^T for a < b)
//   Sigma_{k,k}     = F_k^T F_k - sum_{I < cnt} G_I^T Sigma_{k+1+I,k}
// Only blocks inside the block band are touched, so the result is exact on the band; the cost is O(n W^2) like the sweep's.
#pragma once
#include "sf_band_solve.h"

// One workgroup per matrix, one wave per block below the diagonal (sfb_selinv_nwaves).  The Sigma blocks of the last nbr - 1
// block columns live in LDS (sfb_selinv_lds_layout); the factor's block column comes from global memory straight into MFMA
// operand registers, column k - 1 requested before this step's sums are issued.  Per step k:
//   wave I < cnt   G_I = L_{k+1+I,k} F_k                                                      -> G[I]
//   barrier
//   wave J < cnt   Sigma_{k+1+J,k} = - sum_I Sigma_{k+1+J,k+1+I} G_I, I ascending             -> its slot of S, and out
//                  P_J = G_J^T Sigma_{k+1+J,k}                                                -> P[J]
//   barrier
//   wave 0         Sigma_kk = F_k^T F_k - P_0 - P_1 - ..., mirrored from its lower triangle   -> its slot of S, and out
// (wave 0 goes on to G_0 of column k - 1 while the others wait at the next barrier: neither G nor P of step k is read any
// more by then).  Every sum has one order, whatever the batch.  A matrix with info != 0 gets NaN and nothing of it is read.
struct sf_band_selinv_args {
    const double* fac;  // the keeping sweep's records
    int64_t sfac;
    const int* info;    // [batch]
    double* out;        // out[b * sout + i * ldo + d] = Sigma[i][i - d], 0 <= d <= min(i, halfwidth), i < n
    int64_t sout;
    int ldo, n, nbr, nrb, halfwidth;
};
__global__ __launch_bounds__(64 * SFB_SELINV_MAX_WAVES) void k_band_selinv(sf_band_selinv_args a) {
    extern __shared__ double lds[];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lq = lane >> 4;
    const int n = a.n, nbr = a.nbr, nrb = a.nrb, nb1 = nbr - 1, nblk = (n + BB - 1) / BB, W = a.halfwidth;
    double* out = a.out + (int64_t)b * a.sout;
    if (a.info[b] != 0) {
        for (int e = tid; e < n * (W + 1); e += blockDim.x) {
            const int i = e / (W + 1), d = e - i * (W + 1);
            if (d <= i) out[(int64_t)i * a.ldo + d] = __builtin_nan("");
        }
        return;
    }
    const sfb_selinv_lds L = sfb_selinv_lds_layout(nbr);
    double* S = lds + L.S;
    double* G = lds + L.G;
    double* P = lds + L.P;
    const double* fac = a.fac + (int64_t)b * a.sfac;
    const int oA = l15 * BLD + 4 * lq;  // X[l15][4 lq + kk] of a stored block: A operand, or B operand of its transpose
    const int oT = 4 * lq * BLD + l15;  // X[4 lq + kk][l15] (kk rows apart): B operand, or A operand of its transpose
    const int oD = lq * BLD + l15;      // accumulator rows lq + 4 r
    auto wrap = [&](int slot) { return slot >= nbr ? slot - nbr : slot; };  // slot in [0, 2 nbr)

    sf_d4 Lr = {0.0, 0.0, 0.0, 0.0}, Fr;  // this wave's L_{k+1+wave,k} as A operand, F_k as B operand (= F_k^T as A operand)
    auto request = [&](int k) {
        const double* Fb = fac + sfb_keep_block(k, 0, nbr, nrb) + 4 * lq * BB + l15;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) Fr[kk] = Fb[kk * BB];
        if (wave < min(nb1, nblk - 1 - k)) {
            const double* Lb = fac + sfb_keep_block(k, 1 + wave, nbr, nrb) + l15 * BB + 4 * lq;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) Lr[kk] = Lb[kk];
        }
    };
    request(nblk - 1);
    int ks = (nblk - 1) % nbr;  // ring slot of block column k
    for (int k = nblk - 1; k >= 0; --k, ks = ks == 0 ? nbr - 1 : ks - 1) {
        const int cnt = min(nb1, nblk - 1 - k);
        const sf_d4 Fk = Fr;
        if (wave < cnt) {
            sf_d4 g = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) g = __builtin_amdgcn_mfma_f64_16x16x4f64(Lr[kk], Fk[kk], g, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) G[wave * BS + oD + 4 * r * BLD] = g[r];
        }
        if (k > 0) request(k - 1);  // lands under the rest of this step
        __syncthreads();
        if (wave < cnt) {
            const int J = wave, sj = wrap(ks + 1 + J);
            sf_d4 acc = {0.0, 0.0, 0.0, 0.0};
            for (int I = 0; I < cnt; ++I) {
                const double* X = S + sfb_pair(sj, wrap(ks + 1 + I)) * BS;  // the stored block has the later block's rows
                const double* Ap = X + (J >= I ? oA : oT);
                const int as = J >= I ? 1 : BLD;
                const double* Bp = G + I * BS + oT;
#pragma unroll
                for (int kk = 0; kk < 4; ++kk)
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Ap[kk * as], Bp[kk * BLD], acc, 0, 0, 1);  // neg: -A B + C
            }
            double* D = S + sfb_pair(sj, ks) * BS;
            const int col = k * BB + l15;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = (k + 1 + J) * BB + lq + 4 * r;
                D[oD + 4 * r * BLD] = acc[r];
                if (row < n && row - col <= W) out[(int64_t)row * a.ldo + (row - col)] = acc[r];
            }
            __builtin_amdgcn_wave_barrier();  // (the wave reads back what its own lanes wrote: LDS serves a wave in order)
            sf_d4 p = {0.0, 0.0, 0.0, 0.0};
            const double* Gj = G + J * BS + oT;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) p = __builtin_amdgcn_mfma_f64_16x16x4f64(Gj[kk * BLD], D[oT + kk * BLD], p, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) P[J * BS + oD + 4 * r * BLD] = p[r];
        }
        __syncthreads();
        if (wave == 0) {
            sf_d4 t = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) t = __builtin_amdgcn_mfma_f64_16x16x4f64(Fk[kk], Fk[kk], t, 0, 0, 0);
            for (int I = 0; I < cnt; ++I)
#pragma unroll
                for (int r = 0; r < 4; ++r) t[r] -= P[I * BS + oD + 4 * r * BLD];
            double* D = S + sfb_pair(ks, ks) * BS;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int rr = lq + 4 * r, row = k * BB + rr;
                if (rr >= l15) {  // the lower triangle, mirrored: the block is read from either side
                    D[rr * BLD + l15] = t[r];
                    D[l15 * BLD + rr] = t[r];
                    if (row < n && rr - l15 <= W) out[(int64_t)row * a.ldo + (rr - l15)] = t[r];
                }
            }
        }
    }
}

// fac: the records of sf_launch_band_keep for the same n, halfwidth and nrhs; out[b * sout + i * ldo + d], ldo >= halfwidth + 1
int sf_launch_band_selinv(const double* fac, int n, int halfwidth, int batch, int nrhs, const int* info, double* out, int ldo,
                          int64_t sout, hipStream_t s) {
    if (!fac || !info || !out || n <= 0 || batch <= 0 || ldo < halfwidth + 1 || sfb_admit(halfwidth, nrhs) != SFB_WINDOW ||
        !sfb_selinv_admits(halfwidth)) {
        sf_set_error("band_selinv: bad arguments, or the half-width exceeds the LDS window (n=%d halfwidth=%d nrhs=%d ldo=%d)", n,
                     halfwidth, nrhs, ldo);
        return SF_EINVAL;
    }
    const int nbr = sfb_nbr(halfwidth), nrb = sfb_nrb(nrhs);
    const size_t shm = sfb_selinv_lds_layout(nbr).bytes;
    static sf_dev_once attr_once;
    SF_CHECK(sf_lds_limit_once(&attr_once, SFB_LDS_MAX, {(const void*)k_band_selinv}));
    const sf_band_selinv_args a = {fac, (int64_t)sfb_keep_doubles(n, nbr, nrb), info, out, sout, ldo, n, nbr, nrb, halfwidth};
    hipLaunchKernelGGL(k_band_selinv, dim3(batch), dim3(64 * sfb_selinv_nwaves(nbr)), shm, s, a);
    SF_LAUNCH_CHECK();
    return SF_OK;
}

// The capacitance matrix S = I + G of one walker (G = gram[kr:, kr:] of the sweep over kr + m rows) into S[r * 33 + c], and its
// factor S = L_S L_S^T in place (lower; the diagonal holds 1 / l_jj), one wave.  The steps of k_band_mix_matrix.
__device__ __forceinline__ void sfb_capacitance_factor(const double* g, int kr, int m, int lane, double* S) {
    const int nrhs = kr + m;
    for (int e = lane; e < m * m; e += 64) {
        const int r = e / m, c = e - r * m;
        S[r * 33 + c] = g[(r + kr) * nrhs + (c + kr)] + (r == c ? 1.0 : 0.0);
    }
    __syncthreads();
    for (int j = 0; j < m; ++j) {
        const double rs = 1.0 / sqrt(S[j * 33 + j]);
        __syncthreads();
        double lij = 0.0;
        if (lane > j && lane < m) {
            lij = S[lane * 33 + j] * rs;
            S[lane * 33 + j] = lij;
        }
        if (lane == j) S[j * 33 + j] = rs;
        __syncthreads();
        if (lane > j && lane < m)
            for (int c = j + 1; c <= lane; ++c) S[lane * 33 + c] -= lij * S[c * 33 + j];
        __syncthreads();
    }
}
// C^-1 = Sigma - Vs Vs^T with Vs = T_Y L_S^-T (n x m): Vs = T M2 through k_band_mix.  T has kr rows in front of the m rows of
// Y; M2 is (kr + m) x (co + m): its first kr rows and first co columns are zero and M2[kr + j][co + c] = (L_S^-1)[c][j].  The
// gradient keeps the staging layout of its mix (kr = co = 1: row 0 of the product is zero), the diagnostics ask for the m
// columns alone (co = 0).  One wave per walker; lane c solves L_S z = e_c, column c of L_S^-1, which is row kr + c of M2.  A
// walker with info != 0 is not read.
__global__ __launch_bounds__(64) void k_band_vs_matrix(const double* __restrict__ gram, int kr, int m, int co,
                                                       const int* __restrict__ info, double* __restrict__ M2) {
    __shared__ double S[33 * 33];
    const int b = blockIdx.x, lane = threadIdx.x, nin = kr + m, nout = co + m;
    if (info[b] != 0) return;
    sfb_capacitance_factor(gram + (int64_t)b * nin * nin, kr, m, lane, S);
    double* Mb = M2 + (int64_t)b * nin * nout;
    if (lane < nout)
        for (int r = 0; r < kr; ++r) Mb[r * nout + lane] = 0.0;
    if (lane < nin)
        for (int c = 0; c < co; ++c) Mb[lane * nout + c] = 0.0;
    if (lane < m) {
        const int c = lane;
        double z[32];
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            double v = j == c ? 1.0 : 0.0;
            if (j < m) {
#pragma unroll
                for (int i = 0; i < j; ++i) v -= S[j * 33 + i] * z[i];
                v *= S[j * 33 + j];
            }
            z[j] = v;
        }
#pragma unroll
        for (int j = 0; j < 32; ++j)
            if (j < m) Mb[(kr + c) * nout + co + j] = z[j];
    }
}
// stage2[b][co + c] = column c of Vs (rows < co are zero), [batch][co + m][npad]: with kr = co = 1 the staging layout of the
// gradient's sf_launch_band_mix
int sf_launch_band_vs(const double* gram, int kr, int m, int co, const int* info, const double* T, int n, int npad, int batch,
                      double* Mwork, double* stage2, hipStream_t s) {
    if (m < 1 || m > 32 || kr < 1 || kr + m > SFB_MIX_MAX || (co != 0 && co != kr) || co + m > SFB_MIX_MAX || batch <= 0 ||
        batch > 65535 || n <= 0 || npad < n) {
        sf_set_error("band_vs: 1 .. 32 low-rank rows, at most %d rows of right-hand sides in all, 1 .. 65535 walkers", SFB_MIX_MAX);
        return SF_EINVAL;
    }
    hipLaunchKernelGGL(k_band_vs_matrix, dim3(batch), dim3(64), 0, s, gram, kr, m, co, info, Mwork);
    SF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_band_mix, dim3((npad + 255) / 256, batch), dim3(256), 0, s, T, Mwork, info, kr + m, kr, co, co + m, n, npad,
                       stage2);
    SF_LAUNCH_CHECK();
    return SF_OK;
}
