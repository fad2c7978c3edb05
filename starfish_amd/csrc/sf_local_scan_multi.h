// The averaged proposal of a score scan (sf_local_scan_mean): what EchelleModel.propose_local_kernels(P=...) reads back per order
// of a multi-order scan (sf_local_scan_banded_multi_batch_md) instead of the walkers' triples.  A layer of sf_transform.hip
// ("Score scan of an echelle model"); the scan itself has no device code of its own -- its kernels are the single-order
// call's (sf_band_local_scan.h, sf_local_scan.h), launched per segment behind the chunk's sweeps.
//   mean       k_ls_mean: one thread per candidate q.  Per walker b with info[b] == 0, ascending: U = (quad - trace) / 2, z = U /
//              sqrt(fisher), amp = U / fisher (NaN where fisher == 0: no pixel in reach), s = v_0; s = s + v_1; ...; then the two
//              sums divided by the number of walkers used (none: NaN).  Neighbouring threads read neighbouring triples of a
//              walker's row.  Thread 0 writes the count.  Plain adds, no atomics.
#pragma once

__global__ __launch_bounds__(256) void k_ls_mean(int B, int ncand, const double* __restrict__ out, const int* __restrict__ info,
                                                 double* __restrict__ mean, int* __restrict__ count) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= ncand) return;
    double sz = 0.0, sa = 0.0;
    int used = 0;
    for (int b = 0; b < B; ++b) {
        if (info[b] != 0) continue;
        const double* __restrict__ t = out + ((int64_t)b * ncand + q) * 3;
        const double quad = t[0], trace = t[1], fisher = t[2];
        const double U = 0.5 * (quad - trace);
        const double z = fisher == 0.0 ? __builtin_nan("") : U / sqrt(fisher);
        const double amp = fisher == 0.0 ? __builtin_nan("") : U / fisher;
        sz = used ? sz + z : z;
        sa = used ? sa + amp : amp;
        ++used;
    }
    mean[2 * q] = used ? sz / (double)used : __builtin_nan("");
    mean[2 * q + 1] = used ? sa / (double)used : __builtin_nan("");
    if (q == 0) *count = used;
}
int sf_launch_local_scan_mean(int B, int ncand, const double* out, const int* info, double* mean, int* count, hipStream_t s) {
    if (!out || !info || !mean || !count || B < 1 || ncand < 1) {
        sf_set_error("sf_local_scan_mean: the triples, the status, the outputs, B >= 1 and ncand >= 1 are required");
        return SF_EINVAL;
    }
    hipLaunchKernelGGL(k_ls_mean, dim3((unsigned)((ncand + 255) / 256)), dim3(256), 0, s, B, ncand, out, info, mean, count);
    SF_LAUNCH_CHECK();
    return SF_OK;
}
