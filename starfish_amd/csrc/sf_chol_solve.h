// After the factorisation: logdet and Mahalanobis term from L and z (k_logdet_z), the stand-alone forward substitution
// of sf_logdet_sqmah_batch (k_trsv_logdet), and the clock probe of the tuning scripts.  Independent of the sequences.
#pragma once
#include "sf_device.h"

// One workgroup per matrix: forward substitution L z = R by 64-row blocks (left-looking: the
// row block is read once, coalesced), then logdet = 2 sum log L_ii and sqmah = z.z.
template <bool ZGLOBAL>
__global__ __launch_bounds__(256) void k_trsv_logdet(const double* __restrict__ base, int n, int lda,
                                                     int64_t stride, const double* __restrict__ R,
                                                     int ldr, double* __restrict__ zscratch,
                                                     double* __restrict__ logdet,
                                                     double* __restrict__ sqmah) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    double* Ts = sm;                     // 64 x 65 diagonal block
    double* tv = Ts + SF_LEAF * 65;      // 64 right-hand sides of the block
    double* red = tv + SF_LEAF;          // 8 reduction slots
    double* z = ZGLOBAL ? zscratch + (int64_t)blockIdx.x * n : red + 8;

    const int b = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, w = tid >> 6;
    const double* Mx = base + (int64_t)b * stride;
    const double* Rb = R + (int64_t)b * ldr;

    for (int c = 0; c < n; c += SF_LEAF) {
        for (int e = tid; e < SF_LEAF * SF_LEAF; e += 256) {
            const int i = e >> 6, j = e & 63;
            Ts[i * 65 + j] = Mx[(int64_t)(c + i) * lda + c + j];
        }
        // 16 rows per wave, all 16 row streams in flight together
        double s[16];
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) s[rr] = 0.0;
        const double* prow = Mx + (int64_t)(c + w * 16) * lda;
        for (int k = lane; k < c; k += 64) {
            const double zk = z[k];
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) s[rr] += prow[(int64_t)rr * lda + k] * zk;
        }
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const double tot = sf_wave_sum(s[rr]);
            if (lane == 0) tv[w * 16 + rr] = Rb[c + w * 16 + rr] - tot;
        }
        __syncthreads();
        if (w == 0) {
            double tval = tv[lane];
#pragma unroll 8
            for (int k = 0; k < SF_LEAF; ++k) {
                const double zk = __shfl(tval, k) / Ts[k * 65 + k];
                if (lane > k)
                    tval -= Ts[lane * 65 + k] * zk;
                else if (lane == k)
                    tval = zk;
            }
            z[c + lane] = tval;
        }
        __syncthreads();
    }
    double slog = 0.0, ssq = 0.0;
    for (int i = tid; i < n; i += 256) {
        slog += log(Mx[(int64_t)i * lda + i]);
        const double zi = z[i];
        ssq += zi * zi;
    }
    slog = sf_wave_sum(slog);
    ssq = sf_wave_sum(ssq);
    if (lane == 0) {
        red[w] = slog;
        red[4 + w] = ssq;
    }
    __syncthreads();
    if (tid == 0) {
        logdet[b] = 2.0 * (red[0] + red[1] + red[2] + red[3]);
        sqmah[b] = red[4] + red[5] + red[6] + red[7];
    }
}

// One workgroup per matrix: logdet = 2 sum log L_ii and sqmah = |z|^2 where z = L^-1 R was produced
// in place of R by the factorisation.
__global__ __launch_bounds__(256) void k_logdet_z(const double* __restrict__ base, int n, int lda,
                                                  int64_t stride, const double* __restrict__ zbuf, int ldr,
                                                  double* __restrict__ logdet,
                                                  double* __restrict__ sqmah) {
    __shared__ double red[8];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const double* Mx = base + (int64_t)b * stride;
    const double* z = zbuf ? zbuf + (int64_t)b * ldr : nullptr;
    double slog = 0.0, ssq = 0.0;
    for (int i = tid; i < n; i += 256) {
        slog += log(Mx[(int64_t)i * lda + i]);
        const double zi = z ? z[i] : 0.0;
        ssq += zi * zi;
    }
    slog = sf_wave_sum(slog);
    ssq = sf_wave_sum(ssq);
    if (lane == 0) {
        red[w] = slog;
        red[4 + w] = ssq;
    }
    __syncthreads();
    if (tid == 0) {
        logdet[b] = 2.0 * (red[0] + red[1] + red[2] + red[3]);
        sqmah[b] = red[4] + red[5] + red[6] + red[7];
    }
}

int sf_launch_logdet_z(const double* L, int n, int lda, int64_t stride, int batch, const double* z, int ldr,
                       double* logdet, double* sqmah, hipStream_t s) {
    hipLaunchKernelGGL(k_logdet_z, dim3(batch), dim3(256), 0, s, L, n, lda, stride, z, ldr, logdet, sqmah);
    SF_LAUNCH_CHECK();
    return SF_OK;
}

int sf_launch_logdet_sqmah(const double* L, int n, int lda, int64_t stride, int batch, const double* R,
                           int ldr, double* zscratch, double* logdet, double* sqmah, hipStream_t s) {
    if (n % SF_LEAF != 0 || batch <= 0) {
        sf_set_error("logdet_sqmah: n must be a multiple of %d", SF_LEAF);
        return SF_EINVAL;
    }
    const size_t fixed = sizeof(double) * (SF_LEAF * 65 + SF_LEAF + 8);
    const size_t with_z = fixed + sizeof(double) * (size_t)n;
    if (with_z <= 160 * 1024) {
        static sf_dev_once attr_once;  // devices whose function attributes are set
        SF_CHECK(sf_lds_limit_once(&attr_once, 160 * 1024, {(const void*)k_trsv_logdet<false>}));
        hipLaunchKernelGGL(k_trsv_logdet<false>, dim3(batch), dim3(256), with_z, s, L, n, lda, stride, R,
                           ldr, (double*)nullptr, logdet, sqmah);
    } else {
        if (!zscratch) {
            sf_set_error("logdet_sqmah: n=%d needs a z scratch buffer", n);
            return SF_ENOMEM;
        }
        hipLaunchKernelGGL(k_trsv_logdet<true>, dim3(batch), dim3(256), fixed, s, L, n, lda, stride, R, ldr,
                           zscratch, logdet, sqmah);
    }
    SF_LAUNCH_CHECK();
    return SF_OK;
}

// Debug aid for the tuning scripts: one wave spins for `wall_ticks` ticks of the 100 MHz wall clock and
// reports how many shader-clock ticks (s_memtime) elapsed -> sustained shader clock while other
// streams are busy.  out[0] = s_memtime ticks, out[1] = wall ticks.
__global__ void k_clock_probe(long long* out, long long wall_ticks) {
    const long long w0 = wall_clock64();
    const long long t0 = __builtin_amdgcn_s_memtime();
    long long w1 = w0;
    while (w1 - w0 < wall_ticks) {
        __builtin_amdgcn_s_sleep(32);
        w1 = wall_clock64();
    }
    const long long t1 = __builtin_amdgcn_s_memtime();
    if (threadIdx.x == 0) {
        out[0] = t1 - t0;
        out[1] = w1 - w0;
    }
}
int sf_launch_clock_probe(long long* out, long long wall_ticks, hipStream_t s) {
    hipLaunchKernelGGL(k_clock_probe, dim3(1), dim3(64), 0, s, out, wall_ticks);
    SF_LAUNCH_CHECK();
    return SF_OK;
}
