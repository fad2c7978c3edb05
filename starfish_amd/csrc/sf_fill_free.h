// Stand-alone kernels (free functions of the ABI) and the streaming-write probe.
#pragma once

__global__ __launch_bounds__(256) void k_global_cov(const double* __restrict__ wave, int n, double amp,
                                                    double ls, double* __restrict__ out) {
    const int col = blockIdx.x * 256 + threadIdx.x, row = blockIdx.y;
    if (col >= n) return;
    out[(int64_t)row * n + col] = sf_matern_elem(wave[row], wave[col], amp, ls, 6 * ls);
}

__global__ __launch_bounds__(256) void k_local_cov(const double* __restrict__ wave, int n, double amp,
                                                   double mu, double sigma, int accumulate,
                                                   double* __restrict__ out) {
    const int col = blockIdx.x * 256 + threadIdx.x, row = blockIdx.y;
    if (col >= n) return;
    const double v = sf_local_elem(sf_local_metric(wave[row], mu), sf_local_metric(wave[col], mu), amp,
                                   sigma, 4 * sigma);
    double* o = out + (int64_t)row * n + col;
    *o = accumulate ? (*o + v) : v;
}

int sf_launch_global_cov(const double* wave, int n, double amp, double ls, double* out, hipStream_t s) {
    if (n <= 0) return SF_OK;
    hipLaunchKernelGGL(k_global_cov, dim3((n + 255) / 256, n), dim3(256), 0, s, wave, n, amp, ls, out);
    SF_LAUNCH_CHECK();
    return SF_OK;
}

int sf_launch_local_cov(const double* wave, int n, double amp, double mu, double sigma, int accumulate,
                        double* out, hipStream_t s) {
    if (n <= 0) return SF_OK;
    hipLaunchKernelGGL(k_local_cov, dim3((n + 255) / 256, n), dim3(256), 0, s, wave, n, amp, mu, sigma,
                       accumulate, out);
    SF_LAUNCH_CHECK();
    return SF_OK;
}

// Streaming-write probe (sf_debug_stream_write): every lane stores 16 bytes per iteration, a workgroup covers a contiguous
// 64 KB chunk per iteration (the write pattern of a bandwidth test, no reads).
__global__ __launch_bounds__(256) void k_stream_write(double* __restrict__ dst, size_t count2, double v) {
    double2* __restrict__ d2 = (double2*)dst;
    const double2 val = make_double2(v, v);
    const size_t chunk = 4096;  // double2 per workgroup and iteration
    for (size_t base = (size_t)blockIdx.x * chunk; base < count2; base += (size_t)gridDim.x * chunk) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const size_t j = base + (size_t)i * 256 + threadIdx.x;
            if (j < count2) d2[j] = val;
        }
    }
}
int sf_launch_stream_write(double* dst, size_t count, double v, hipStream_t s) {
    if (((uintptr_t)dst & 15) != 0 || (count & 1)) {
        sf_set_error("stream write probe: 16-byte aligned destination and an even count");
        return SF_EINVAL;
    }
    const size_t count2 = count / 2;
    if (!count2) return SF_OK;
    const unsigned grid = (unsigned)std::min<size_t>((count2 + 4095) / 4096, 256 * 32);
    hipLaunchKernelGGL(k_stream_write, dim3(grid), dim3(256), 0, s, dst, count2, v);
    SF_LAUNCH_CHECK();
    return SF_OK;
}
