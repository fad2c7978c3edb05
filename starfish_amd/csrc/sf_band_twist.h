// The two-sided ("twisted") sweep: two half sweeps, k_band_merge, and a short sweep over the separator.
#pragma once
#include "sf_band_sweep.h"

// Merge of the two half sweeps: separator = top + flip(bottom) - A_MM (A_MM is contained in both dumps),
// written in band storage (half-width nm-1) so that the ordinary single sweep finishes the job.
__global__ __launch_bounds__(256) void k_band_merge(sf_band_args a, int nm, int NR, int row0, double* mband,
                                                    double* mrhs, double* gadd, double* ladd) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const double* band = a.band + (int64_t)b * a.sband;
    const double* top = a.dumpM + ((int64_t)b * 2) * nm * nm;
    const double* bot = top + (int64_t)nm * nm;
    double* mb = mband + (int64_t)b * nm * nm;
    for (int e = tid; e < nm * nm; e += 256) {
        const int i = e / nm, j = e - i * nm;
        if (j > i) continue;
        const int d = i - j;
        const double aij = d <= a.halfwidth ? band[(int64_t)(row0 + i) * a.ldb + d] : 0.0;
        mb[i * nm + d] = top[i * nm + j] + bot[(nm - 1 - j) * nm + (nm - 1 - i)] - aij;
    }
    const double* rt = a.dumpR + ((int64_t)b * 2) * NR * nm;
    const double* rb = rt + (int64_t)NR * nm;
    double* mr = mrhs + (int64_t)b * NR * nm;
    for (int e = tid; e < NR * nm; e += 256) {
        const int r = e / nm, j = e - r * nm;
        const double orig = r < a.r.nrhs ? a.r.of(b).row(r)[row0 + j] : 0.0;
        mr[e] = rt[e] + rb[r * nm + (nm - 1 - j)] - orig;
    }
    const int ng = a.r.nrhs * a.r.nrhs;
    const double* gt = a.dumpG + ((int64_t)b * 2) * ng;
    for (int e = tid; e < ng; e += 256) gadd[(int64_t)b * ng + e] = gt[e] + gt[ng + e];
    if (tid == 0) ladd[b] = a.dumpL[2 * b] + a.dumpL[2 * b + 1];
}

// Whether two half sweeps pay for this batch on the current device (the rule: sfb_twist_pays)
bool sf_band_twisted_applicable(int n, int halfwidth, int batch) {
    static int ncu = 0;
    if (!ncu) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
            ncu = 1;
    }
    return n % BB == 0 && sfb_twist_pays(n / BB, sfb_nbr(halfwidth), batch, ncu);
}

// Two workgroups per matrix: top-down and bottom-up half sweeps meet at a separator of nm = 16*(nbr-1)
// rows, which a third (short) sweep finishes.  Pays off while 2*batch workgroups still fit the chip (the
// sweep is a sequential chain, so halving it halves the latency) and whenever it fills the rounds better.  `work` needs
// sfb_twist_carve(...).doubles doubles.
int sf_launch_band_forms_twisted(const sf_band_call& c, double* work, hipStream_t s) {
    const int nrhs = c.r.nrhs, NR = sfb_nrb(nrhs) * BB, nbr = sfb_nbr(c.halfwidth), nblk = c.n / BB;
    if (c.n % BB || !sfb_twist_fits(nblk, nbr) || sfb_admit(c.halfwidth, nrhs) != SFB_WINDOW || c.ldb < c.halfwidth + 1) {
        sf_set_error("band_forms_twisted: bad arguments");
        return SF_EINVAL;
    }
    const sfb_twist t = sfb_twist_shape(nblk, nbr);
    const sfb_twist_work w = sfb_twist_carve(work, c.halfwidth, nrhs, c.batch);
    sf_band_args a = band_args(c);  // no results: the halves dump
    a.nhalf = 2;
    a.kend0 = t.kend0, a.kend1 = t.kend1;
    a.dumpM = w.dumpM, a.dumpR = w.dumpR, a.dumpG = w.dumpG, a.dumpL = w.dumpL;
    int rc = launch_forms_kernel(a, 2 * c.batch, s);
    if (rc) return rc;
    hipLaunchKernelGGL(k_band_merge, dim3(c.batch), dim3(256), 0, s, a, t.nm, NR, t.kend0 * BB, w.mband, w.mrhs, w.gadd, w.ladd);
    SF_LAUNCH_CHECK();
    // the separator: a dense nm x nm matrix in band storage (half-width nm-1 -> the same window size)
    sf_band_call sep = c;
    sep.band = w.mband, sep.sband = (int64_t)t.nm * t.nm, sep.ldb = t.nm, sep.halfwidth = t.nm - 1, sep.n = t.nm;
    sep.r = sf_band_rhs{w.mrhs, (int64_t)NR * t.nm, t.nm, nrhs, nullptr, 0};
    return launch_band_forms(sep, w.ladd, w.gadd, t.kend0 * BB, s);
}
