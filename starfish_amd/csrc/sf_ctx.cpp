// Context creation: the constants of one order (collocation factor of the fixed log-lambda grid, static spline coefficients
// and half spectra) and of the emulator (factor of the constant v11) are prepared once and kept on the device.
#include <vector>

#include "sf_ctx.h"
#include "sf_hostmath.h"

extern "C" int sf_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" sf_ctx* sf_ctx_create(const sf_order_desc* d, int device, int* err) {
    int rc_dummy = 0;
    int& rc = err ? *err : rc_dummy;
    rc = SF_OK;
    auto fail = [&](int code) -> sf_ctx* {
        rc = code;
        return nullptr;
    };
    // n == 0 builds an emulator-only context (Emulator.__call__ without a SpectrumModel)
    const bool order_ok = d && (d->n == 0 || (d->n >= 2 && d->nf >= 8 && !(d->nf & (d->nf - 1)) && d->wave &&
                                               d->flux && d->sigma && d->min_dv_wave && d->bulk_fluxes));
    if (d && (d->m < 1 || d->m > SF_MAX_M)) {
        sf_set_error("sf_ctx_create: %d eigenspectra, between 1 and %d (SF_MAX_M) are supported", d->m, SF_MAX_M);
        return fail(SF_EINVAL);
    }
    if (!d || !order_ok || d->m < 1 || d->m > SF_MAX_M || d->n_grid < 1 || d->M < 1 || !d->grid_points ||
        !d->variances || !d->lengthscales || !d->v11 || !d->w_hat) {
        sf_set_error("sf_ctx_create: bad descriptor");
        return fail(SF_EINVAL);
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device) {
        sf_set_error("sf_ctx_create: no HIP device %d", device);
        return fail(SF_ENODEV);
    }
    if (hipSetDevice(device) != hipSuccess) {
        sf_set_error("hipSetDevice(%d) failed", device);
        return fail(SF_EHIP);
    }
    sf_ctx* c = new sf_ctx();
    c->device = device;
    c->n = d->n;
    c->nf = d->nf;
    c->m = d->m;
    c->P = d->n_grid;
    c->M = d->M;
    c->rows = d->m + 2;
    c->npad = (int)sf_align_up((size_t)d->n, SF_LEAF);
    c->lda = c->npad + 16;  // breaks the power-of-two row stride (HBM channel camping)
    c->mpad = (int)sf_align_up((size_t)d->m, 4);
    const bool has_order = d->n > 0;
    c->dv = has_order ? min_dv(d->min_dv_wave, d->nf) : 0.0;
    c->wave_max = has_order ? d->wave[0] : 0.0;
    for (int i = 0; i < d->n; ++i) {
        if (d->wave[i] > c->wave_max) c->wave_max = d->wave[i];
        if (i && !(d->wave[i] > d->wave[i - 1])) c->monotonic = 0;
    }
    if (c->monotonic && d->n > 2) c->loguniform = is_loguniform(d->wave, d->n);
#define TRY(x)              \
    do {                    \
        int rc__ = (x);     \
        if (rc__) {         \
            delete c;       \
            return fail(rc__); \
        }                   \
    } while (0)
    const size_t nb = sizeof(double) * (size_t)d->n;
    if (has_order) {
    TRY(c->wave.upload(d->wave, nb));
    TRY(c->flux.upload(d->flux, nb));
    TRY(c->sigma.upload(d->sigma, nb));

    std::vector<double> t, Lf, Uf, rdiag, tw;
    TRY(quintic_collocation_lu(d->min_dv_wave, d->nf, t, Lf, Uf, rdiag));
    TRY(c->knots.upload(t.data(), sizeof(double) * t.size()));
    TRY(c->Lf.upload(Lf.data(), sizeof(double) * Lf.size()));
    TRY(c->Uf.upload(Uf.data(), sizeof(double) * Uf.size()));
    TRY(c->rdiag.upload(rdiag.data(), sizeof(double) * rdiag.size()));
    {
        std::vector<double> band, tblk;
        truncated_inverse_band(d->nf, Lf, Uf, rdiag, band);
        inverse_band_blocks(d->nf, band, tblk);
        TRY(c->inv_band.upload(tblk.data(), sizeof(double) * tblk.size()));
    }
    make_twiddles(d->nf, tw);
    TRY(c->tw.upload(tw.data(), sizeof(double) * tw.size()));

    // static spline coefficients of the un-broadened rows, stored [nf][rows]
    {
        std::vector<double> ct((size_t)d->nf * c->rows);
        for (int r = 0; r < c->rows; ++r)
            for (int j = 0; j < d->nf; ++j) ct[(size_t)j * c->rows + r] = d->bulk_fluxes[(size_t)r * d->nf + j];
        TRY(c->coef_static.upload(ct.data(), sizeof(double) * ct.size()));
        TRY(sf_launch_spline_solve(c->coef_static.as<double>(), 1, c->rows, 0, 1, c->rows, d->nf,
                                   c->Lf.as<double>(), c->Uf.as<double>(), c->rdiag.as<double>(), 0));
    }
    // half spectra of the static rows (rfft once; every walker only multiplies and inverts)
    {
        DevBuf bulk, scratch;
        TRY(bulk.upload(d->bulk_fluxes, sizeof(double) * (size_t)c->rows * d->nf));
        TRY(c->spec.alloc(sizeof(double2) * (size_t)c->rows * (d->nf / 2 + 1)));
        const size_t sb = sf_fft_scratch_bytes(c->rows, d->nf);
        if (sb) TRY(scratch.alloc(sb));
        TRY(sf_launch_rfft_rows(bulk.as<double>(), c->rows, d->nf, c->tw.as<double2>(), c->spec.as<double2>(),
                                scratch.as<double2>(), 0));
        if (hipDeviceSynchronize() != hipSuccess) {
            sf_set_error("context set-up kernels failed: %s", hipGetErrorString(hipGetLastError()));
            delete c;
            return fail(SF_EHIP);
        }
    }
    }  // has_order
    // emulator constants
    {
        const int N = d->m * d->M;
        std::vector<double> alpha, Linv, gmin(d->n_grid), gmax(d->n_grid);
        if ((d->linv != nullptr) != (d->alpha != nullptr)) {
            sf_set_error("sf_ctx_create: linv and alpha must be given together");
            delete c;
            return fail(SF_EINVAL);
        }
        if (d->linv) {
            Linv.assign(d->linv, d->linv + (size_t)N * N);
            alpha.assign(d->alpha, d->alpha + N);
        } else {
            TRY(emulator_constants(d->v11, d->w_hat, N, alpha, Linv));
        }
        for (int p = 0; p < d->n_grid; ++p) {
            gmin[p] = gmax[p] = d->grid_points[p];
            for (int j = 1; j < d->M; ++j) {
                const double v = d->grid_points[(size_t)j * d->n_grid + p];
                if (v < gmin[p]) gmin[p] = v;
                if (v > gmax[p]) gmax[p] = v;
            }
        }
        TRY(c->grid.upload(d->grid_points, sizeof(double) * (size_t)d->M * d->n_grid));
        TRY(c->variances.upload(d->variances, sizeof(double) * d->m));
        TRY(c->lengthscales.upload(d->lengthscales, sizeof(double) * (size_t)d->m * d->n_grid));
        TRY(c->gmin.upload(gmin.data(), sizeof(double) * d->n_grid));
        TRY(c->gmax.upload(gmax.data(), sizeof(double) * d->n_grid));
        TRY(c->alpha.upload(alpha.data(), sizeof(double) * N));
        {
            // the batched product reads Linv by columns: store the transpose (row index fastest)
            std::vector<double> LinvT((size_t)N * N);
            for (int i = 0; i < N; ++i)
                for (int j = 0; j < N; ++j) LinvT[(size_t)j * N + i] = Linv[(size_t)i * N + j];
            TRY(c->Linv.upload(LinvT.data(), sizeof(double) * (size_t)N * N));
        }
    }
#undef TRY
    return c;
}

extern "C" void sf_ctx_destroy(sf_ctx* c) { delete c; }
extern "C" int sf_ctx_npad(const sf_ctx* c) { return c ? c->npad : SF_EINVAL; }
extern "C" int sf_ctx_lda(const sf_ctx* c) { return c ? c->lda : SF_EINVAL; }

int model_ok(const sf_ctx* c, const sf_model_desc* mdl) {
    if (!c || !mdl || mdl->n_local < 0 || mdl->n_cheb < 0) {
        sf_set_error("bad context / model descriptor");
        return SF_EINVAL;
    }
    if (mdl->n_local > SF_MAX_LOCAL) {
        sf_set_error("%d local kernels: at most %d (SF_MAX_LOCAL) are supported", mdl->n_local, SF_MAX_LOCAL);
        return SF_EINVAL;
    }
    // the broadening runs a half-length transform (at most 65536 points in all) and the spline fit of its rows takes
    // 16-point blocks: refused here, before a batch call enqueues anything, not by the launches themselves
    if (mdl->has_vsini && c->n && (c->nf < SF_NF_MIN_VSINI || c->nf > SF_NF_MAX_VSINI)) {
        sf_set_error("nf=%d: a model with vsini needs %d <= nf <= %d (SF_NF_MIN_VSINI, SF_NF_MAX_VSINI)", c->nf,
                     SF_NF_MIN_VSINI, SF_NF_MAX_VSINI);
        return SF_EINVAL;
    }
    return SF_OK;
}
// the calling thread's current device becomes the context's (HIP's current device is per thread)
int use_device(const sf_ctx* c) {
    SF_HIP(hipSetDevice(c->device));
    return SF_OK;
}
extern "C" int sf_param_stride(const sf_ctx* c, const sf_model_desc* mdl) {
    if (model_ok(c, mdl)) return SF_EINVAL;
    return 6 + c->P + mdl->n_cheb + 3 * mdl->n_local + (mdl->has_av ? 1 : 0);
}
