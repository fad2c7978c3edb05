// The order / emulator context of the C-ABI (internal): device-resident constants of one order and its executors.
#pragma once
#include "sf_common.h"
#include "sf_transform.h"

struct DevBuf {
    void* p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    int alloc(size_t bytes) {
        SF_HIP(hipMalloc(&p, bytes ? bytes : 8));
        return SF_OK;
    }
    int upload(const void* src, size_t bytes) {
        int rc = alloc(bytes);
        if (rc) return rc;
        SF_HIP(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
        return SF_OK;
    }
    template <typename T>
    T* as() const {
        return (T*)p;
    }
};

struct sf_ctx {
    int device = 0;
    int n = 0, nf = 0, m = 0, P = 0, M = 0, npad = 0, lda = 0, mpad = 0, rows = 0;
    int monotonic = 1;
    int loguniform = 0;  // wave_i = wave_0 e^(i delta) to the rounding of the grid
    double dv = 0.0, wave_max = 0.0;
    DevBuf wave, flux, sigma, knots, spec, tw, Lf, Uf, rdiag, coef_static, inv_band;
    DevBuf grid, variances, lengthscales, gmin, gmax, alpha, Linv;  // (Linv holds the TRANSPOSE of Lc^-1)
    sf_exec exec;        // side / auxiliary streams and the event pool of this context's launch sequences
    sf_exec exec_potrf;  // multi-order calls: the factorisation's own streams / events (exec pipelines the fills)
    ~sf_ctx() {
        sf_exec_release(&exec);
        sf_exec_release(&exec_potrf);
    }
};

#pragma GCC visibility push(hidden)  // shared between the host layer's translation units, not part of the library's surface
int model_ok(const sf_ctx* c, const sf_model_desc* mdl);
// the calling thread's current device becomes the context's (HIP's current device is per thread)
int use_device(const sf_ctx* c);
#pragma GCC visibility pop
