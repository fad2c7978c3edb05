// The sweep: k_band_forms and its launchers.
#pragma once
#include "sf_band_window.h"

// Thread roles (blockDim = 512, 768 or 1024):
//   wave 0       diagonal-block factorisation + inverse (S3), its share of the MFMA work elsewhere
//   waves 1..3   prefetch of the right-hand-side columns, log(pivot), MFMA work
//   waves 4..    prefetch of the band rows (groups of 256 threads = one 16 x 16 block each), MFMA work
// The kernel's text is sf_band_sweep_body.h, compiled twice: here as k_band_forms, and in sf_band_solve.h as k_band_keep, the
// same sweep that also stores what it eliminates.  (Two compilations of one text rather than a template flag: shared
// through an inlined body the existing instantiations came out with another register allocation.)
#define SFB_SWEEP_KERNEL k_band_forms
#define SFB_SWEEP_KEEP 0
#include "sf_band_sweep_body.h"
#undef SFB_SWEEP_KERNEL
#undef SFB_SWEEP_KEEP

static int launch_forms_kernel(const sf_band_args& a, int nblocks, hipStream_t s) {
    const int nbr = a.nbr, nrb = sfb_nrb(a.r.nrhs);
    const size_t shm = sfb_lds_layout(nbr, nrb).bytes;
    static sf_dev_once attr_once;  // devices whose function attributes are set
    SF_CHECK(sf_lds_limit_once(&attr_once, SFB_LDS_MAX,
                               {(const void*)k_band_forms<1>, (const void*)k_band_forms<2>, (const void*)k_band_forms<3>}));
    const int nwaves = sfb_nwaves(nbr);
    if (sfb_loader_groups(nwaves) * SFB_PF < nbr || nwaves * 64 < (nbr - 1 + nrb) * BB) {
        sf_set_error("band_forms: window too large for one workgroup");
        return SF_EINVAL;
    }
    const dim3 blk(nwaves * 64);
    if (nrb == 1) hipLaunchKernelGGL(k_band_forms<1>, dim3(nblocks), blk, shm, s, a);
    else if (nrb == 2) hipLaunchKernelGGL(k_band_forms<2>, dim3(nblocks), blk, shm, s, a);
    else hipLaunchKernelGGL(k_band_forms<3>, dim3(nblocks), blk, shm, s, a);
    SF_LAUNCH_CHECK();
    return SF_OK;
}

// What both launchers pass alike; everything else zero (no results, no additive terms, no sweep halves, no dumps).
static sf_band_args band_args(const sf_band_call& c) {
    sf_band_args a = {};
    a.band = c.band, a.sband = c.sband, a.ldb = c.ldb, a.halfwidth = c.halfwidth;
    a.r = c.r;
    a.n = c.n, a.nbr = sfb_nbr(c.halfwidth);
    a.info = c.info;
    return a;
}

// One sweep per matrix, with the additive terms of a pass over a merged separator (sf_launch_band_forms_twisted) or none
static int launch_band_forms(const sf_band_call& c, const double* logdet_add, const double* gram_add, int info_off, hipStream_t s) {
    const int nrhs = c.r.nrhs, wmax = sf_band_max_halfwidth(nrhs);  // -1: no window takes that many right-hand sides
    if (c.n <= 0 || c.batch <= 0 || c.halfwidth < 0 || c.ldb < c.halfwidth + 1 || wmax < 0) {
        sf_set_error("band_forms: bad arguments (n=%d halfwidth=%d ldb=%d nrhs=%d)", c.n, c.halfwidth, c.ldb, nrhs);
        return SF_EINVAL;
    }
    if (sfb_admit(c.halfwidth, nrhs) != SFB_WINDOW) {
        sf_set_error("band_forms: half-width %d with %d right-hand sides exceeds the LDS window (max %d)", c.halfwidth, nrhs, wmax);
        return SF_EINVAL;
    }
    sf_band_args a = band_args(c);
    a.logdet = c.logdet, a.gram = c.gram;
    a.logdet_add = logdet_add, a.gram_add = gram_add, a.info_off = info_off;
    a.nhalf = 1;
    return launch_forms_kernel(a, c.batch, s);
}
int sf_launch_band_forms(const sf_band_call& c, hipStream_t s) { return launch_band_forms(c, nullptr, nullptr, 0, s); }
