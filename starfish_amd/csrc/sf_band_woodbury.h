// The capacitance step of the Woodbury identity.
#pragma once
#include "sf_common.h"

// Capacitance step of the Woodbury identity, one wave per walker:
//   S = I + gram[1:,1:],  S = L_S L_S^T,  u = L_S^-1 gram[1:,0]
//   logdet = logdet_band + sum log diag(S-pivots),  sqmah = gram[0][0] - u.u
__global__ __launch_bounds__(64) void k_woodbury(const double* __restrict__ gram, int nrhs,
                                                 const double* __restrict__ logdet_band,
                                                 double* __restrict__ logdet, double* __restrict__ sqmah,
                                                 int* __restrict__ info) {
    __shared__ double S[33 * 33];
    __shared__ double u[33];
    const int b = blockIdx.x, lane = threadIdx.x, m = nrhs - 1;
    const double* g = gram + (int64_t)b * nrhs * nrhs;
    for (int e = lane; e < m * m; e += 64) {
        const int r = e / m, c = e - r * m;
        S[r * 33 + c] = g[(r + 1) * nrhs + (c + 1)] + (r == c ? 1.0 : 0.0);
    }
    if (lane < m) u[lane] = g[(lane + 1) * nrhs];
    __syncthreads();
    double ld = 0.0;
    int bad = 0;
    for (int j = 0; j < m; ++j) {
        const double p = S[j * 33 + j];
        if (!(p > 0.0) && !bad) bad = 1;
        const double rs = 1.0 / sqrt(p);
        ld += log(p);
        __syncthreads();
        double lij = 0.0;
        if (lane > j && lane < m) {
            lij = S[lane * 33 + j] * rs;
            S[lane * 33 + j] = lij;
        }
        if (lane == j) u[j] *= rs;  // forward substitution rides along: u_j = (v_j - ...)/l_jj
        __syncthreads();
        if (lane > j && lane < m) {
            for (int c = j + 1; c <= lane; ++c) S[lane * 33 + c] -= lij * S[c * 33 + j];
            u[lane] -= lij * u[j];
        }
        __syncthreads();
    }
    if (lane == 0) {
        double uu = 0.0;
        for (int j = 0; j < m; ++j) uu += u[j] * u[j];
        logdet[b] = logdet_band[b] + ld;
        sqmah[b] = g[0] - uu;
        if (bad && info && info[b] == 0) info[b] = SF_INFO_BAD_WEIGHT_COV;
    }
}

int sf_launch_woodbury(const double* gram, int nrhs, int batch, const double* logdet_band, double* logdet,
                       double* sqmah, int* info, hipStream_t s) {
    if (nrhs < 1 || nrhs > 33) {
        sf_set_error("woodbury: 0..32 low-rank rows supported");
        return SF_EINVAL;
    }
    hipLaunchKernelGGL(k_woodbury, dim3(batch), dim3(64), 0, s, gram, nrhs, logdet_band, logdet, sqmah, info);
    SF_LAUNCH_CHECK();
    return SF_OK;
}
