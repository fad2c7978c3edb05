// FFT broadening: the radix-2 / radix-2^2 FFT bodies, the rotational and instrumental multipliers, k_broaden (full-size,
// free functions and set-up), k_kernel_mult + k_broaden_half (the hot path: half-size inverse transform of precomputed
// half spectra), k_rfft_rows (static rows at context creation) and their launchers.   Starfish/transforms.py:45-134
#pragma once
#include "sf_device.h"
#include "sf_transform.h"

// --------------------------------------------------------------------------------------- FFT
// In-place radix-2 decimation-in-time FFT on `buf` (LDS or global), input already bit-reversed.
// tw[k] = exp(-2 pi i k / nf), k < nf/2; this transform has length L = nf >> shift... (L == nf here)
__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
// log2 of a power of two: FFT stages, bits of a bit-reversed index
__device__ __forceinline__ int sf_log2(int n) {
    int bits = 0;
    while ((1 << bits) < n) ++bits;
    return bits;
}

// `twmul`: the table holds exp(-2 pi i k / (twmul * L)) (a table made for a longer transform).
__device__ void sf_fft_inplace(double2* buf, int L, const double2* __restrict__ tw, bool inverse, int twmul = 1) {
    const int tid = threadIdx.x, nth = blockDim.x;
    int ls = 0;  // log2(half-size)
    for (int s = 1; s < L; s <<= 1, ++ls) {
        const int twstep = L / (2 * s) * twmul;
        for (int idx = tid; idx < L / 2; idx += nth) {
            const int j = idx & (s - 1);
            const int i0 = ((idx >> ls) << (ls + 1)) + j;
            const int i1 = i0 + s;
            double2 wv = tw[j * twstep];
            if (inverse) wv.y = -wv.y;
            const double2 u = buf[i0];
            const double2 v = cmul(wv, buf[i1]);
            buf[i0] = make_double2(u.x + v.x, u.y + v.y);
            buf[i1] = make_double2(u.x - v.x, u.y - v.y);
        }
        __syncthreads();
    }
}

// Same transform with two radix-2 stages fused per pass (radix-2^2): half the LDS sweeps and barriers.
// Input bit-reversed (radix-2 order), output natural, exactly the butterflies of sf_fft_inplace.
__device__ void sf_fft_inplace_r4(double2* buf, int L, const double2* __restrict__ tw, bool inverse, int twmul = 1) {
    const int tid = threadIdx.x, nth = blockDim.x;
    int ls = 0, s = 1;
    if (sf_log2(L) & 1) {  // odd number of stages: one plain radix-2 stage first (half-size 1, twiddle 1)
        for (int idx = tid; idx < L / 2; idx += nth) {
            const double2 u = buf[2 * idx], v = buf[2 * idx + 1];
            buf[2 * idx] = make_double2(u.x + v.x, u.y + v.y);
            buf[2 * idx + 1] = make_double2(u.x - v.x, u.y - v.y);
        }
        __syncthreads();
        s = 2;
        ls = 1;
    }
    for (; s < L; s <<= 2, ls += 2) {
        const int stepA = L / (2 * s) * twmul, stepB = L / (4 * s) * twmul;
        for (int idx = tid; idx < L / 4; idx += nth) {
            const int j = idx & (s - 1);
            const int i0 = ((idx >> ls) << (ls + 2)) + j;
            double2 wA = tw[j * stepA], wB0 = tw[j * stepB], wB1 = tw[(j + s) * stepB];
            if (inverse) {
                wA.y = -wA.y;
                wB0.y = -wB0.y;
                wB1.y = -wB1.y;
            }
            const double2 x0 = buf[i0], x1 = buf[i0 + s], x2 = buf[i0 + 2 * s], x3 = buf[i0 + 3 * s];
            const double2 t1 = cmul(wA, x1), t3 = cmul(wA, x3);
            const double2 a0 = make_double2(x0.x + t1.x, x0.y + t1.y), a1 = make_double2(x0.x - t1.x, x0.y - t1.y);
            const double2 a2 = make_double2(x2.x + t3.x, x2.y + t3.y), a3 = make_double2(x2.x - t3.x, x2.y - t3.y);
            const double2 u2 = cmul(wB0, a2), u3 = cmul(wB1, a3);
            buf[i0] = make_double2(a0.x + u2.x, a0.y + u2.y);
            buf[i0 + 2 * s] = make_double2(a0.x - u2.x, a0.y - u2.y);
            buf[i0 + s] = make_double2(a1.x + u3.x, a1.y + u3.y);
            buf[i0 + 3 * s] = make_double2(a1.x - u3.x, a1.y - u3.y);
        }
        __syncthreads();
    }
}

// Decimation-in-frequency forward FFT: natural-order input, BIT-REVERSED output (so the product
// with a real symmetric multiplier feeds the DIT inverse above without any permutation pass).
__device__ void sf_fft_dif_forward(double2* buf, int L, const double2* __restrict__ tw) {
    const int tid = threadIdx.x, nth = blockDim.x;
    int ls = 0;
    while ((2 << ls) < L) ++ls;  // log2(L/2)
    for (int s = L >> 1; s >= 1; s >>= 1, --ls) {
        const int twstep = L / (2 * s);
        for (int idx = tid; idx < L / 2; idx += nth) {
            const int j = idx & (s - 1);
            const int i0 = ((idx >> ls) << (ls + 1)) + j;
            const int i1 = i0 + s;
            const double2 wv = tw[j * twstep];
            const double2 u = buf[i0], v = buf[i1];
            buf[i0] = make_double2(u.x + v.x, u.y + v.y);
            buf[i1] = cmul(wv, make_double2(u.x - v.x, u.y - v.y));
        }
        __syncthreads();
    }
}

__device__ __forceinline__ unsigned sf_bitrev(unsigned x, int bits) { return __brev(x) >> (32 - bits); }

// Gray (2005) rotational kernel, transforms.py:129-131, and the Gaussian profile, transforms.py:84-85
__device__ __forceinline__ double sf_rot_mult(int k, double val, double vsini) {
    if (k == 0) return 1.0;
    const double freq = k * val;
    const double ub = 2.0 * M_PI * vsini * freq;
    return j1(ub) / ub - 3 * cos(ub) / (2 * (ub * ub)) + 3.0 * sin(ub) / (2 * (ub * ub * ub));
}
__device__ __forceinline__ double sf_inst_mult(int k, double val, double fwhm) {
    const double freq = k * val;
    const double sigma = fwhm / 2.355;
    const double a = M_PI * sigma * freq;
    return exp(-2 * (a * a));
}

static const size_t kLdsFftMax = 8192;  // complex points that fit the 160 KiB LDS (128 KiB)

size_t sf_fft_scratch_bytes(int rows_total, int nf) {  // full-size transform (free functions, set-up)
    return (size_t)nf > kLdsFftMax ? sizeof(double2) * (size_t)rows_total * nf : 0;
}
size_t sf_fft_half_scratch_bytes(int rows_total, int nf) {  // half-size transform of the hot path
    return (size_t)(nf / 2) > kLdsFftMax ? sizeof(double2) * (size_t)rows_total * nf : 0;
}
// Where a transform of L complex points (of rows of nf reals) runs: *shm = its dynamic LDS bytes, with the LDS limit of
// `lds_kernels` raised once per device, or 0: in the caller's global scratch, which has to exist then.
static int sf_fft_place(const char* what, int L, int nf, const void* gscratch, sf_dev_once* once,
                        std::initializer_list<const void*> lds_kernels, size_t* shm) {
    *shm = (size_t)L <= kLdsFftMax ? sizeof(double2) * (size_t)L : 0;
    if (*shm) return sf_lds_limit_once(once, 160 * 1024, lds_kernels);
    if (!gscratch) {
        sf_set_error("%s: nf=%d needs a global FFT scratch buffer", what, nf);
        return SF_ENOMEM;
    }
    return SF_OK;
}

// One workgroup per spectrum row.
//   FWD   : true  -> the row is real input `in` (rows x nf) and is transformed first;
//           false -> `spec` holds the precomputed half spectrum (rows_static x (nf/2+1)).
//   kind  : 0 none (multiplier 1), 1 rotational (param = vsini), 2 instrumental (param = fwhm)
// Output element j of row r of item b is written at out[b*ob + r*orow + j*oelem].
template <bool FWD, bool USE_LDS>
__global__ __launch_bounds__(256) void k_broaden(const double* __restrict__ in,
                                                 const double2* __restrict__ spec, int rows, int nf,
                                                 const double2* __restrict__ tw, double dv, int kind,
                                                 const double* __restrict__ params, int pstride,
                                                 int poff, double scalar_param, double* __restrict__ out,
                                                 int64_t ob, int64_t orow, int64_t oelem,
                                                 double2* __restrict__ gscratch, int* __restrict__ info) {
    extern __shared__ __attribute__((aligned(16))) double2 lbuf[];
    const int row = blockIdx.x, b = blockIdx.y;
    double2* buf = USE_LDS ? lbuf : gscratch + ((int64_t)b * rows + row) * nf;
    const int tid = threadIdx.x;
    const int bits = sf_log2(nf);
    const int nh = nf / 2;

    double param = scalar_param;
    if (params) param = params[(int64_t)b * pstride + poff];
    if (kind == 1 && !(param > 0.0)) {  // transforms.py:121-122
        if (tid == 0 && info) atomicCAS(&info[b], 0, SF_INFO_BAD_VSINI);
        return;
    }
    const double val = 1.0 / (nf * dv);  // numpy.fft.rfftfreq

    if (FWD) {
        const double* x = in + ((int64_t)b * rows + row) * nf;
        for (int j = tid; j < nf; j += 256) buf[j] = make_double2(x[j], 0.0);
        __syncthreads();
        sf_fft_dif_forward(buf, nf, tw);
        // position p holds frequency k = bitrev(p); the multiplier is real and even in k
        for (int p = tid; p < nf; p += 256) {
            const int k = (int)sf_bitrev((unsigned)p, bits);
            const int kk = (k <= nh) ? k : nf - k;
            double mult = 1.0;
            if (kind == 1) mult = sf_rot_mult(kk, val, param);
            else if (kind == 2) mult = sf_inst_mult(kk, val, param);
            double2 X = buf[p];
            X.x *= mult;
            X.y *= mult;
            if (kk == 0 || kk == nh) X.y = 0.0;  // c2r ignores the imaginary part of DC / Nyquist
            buf[p] = X;
        }
    } else {
        // X_k (k <= nf/2) and conj(X_{nf-k}) go straight to their bit-reversed slots
        for (int k = tid; k <= nh; k += 256) {
            double2 X = spec[(int64_t)row * (nh + 1) + k];
            double mult = 1.0;
            if (kind == 1) mult = sf_rot_mult(k, val, param);
            else if (kind == 2) mult = sf_inst_mult(k, val, param);
            X.x *= mult;
            X.y *= mult;
            if (k == 0 || k == nh) X.y = 0.0;
            buf[sf_bitrev(k, bits)] = X;
            if (k != 0 && k != nh) buf[sf_bitrev(nf - k, bits)] = make_double2(X.x, -X.y);
        }
    }
    __syncthreads();
    sf_fft_inplace(buf, nf, tw, true);
    const double inv_n = 1.0 / nf;
    double* o = out + (int64_t)b * ob + (int64_t)row * orow;
    for (int j = tid; j < nf; j += 256) o[(int64_t)j * oelem] = buf[j].x * inv_n;
}

template <bool FWD>
static int launch_broaden_t(const sf_broaden_args& a, hipStream_t s) {
    static sf_dev_once attr_once;  // devices whose function attributes are set
    size_t shm;
    SF_CHECK(sf_fft_place("broaden", a.nf, a.nf, a.gscratch, &attr_once,
                          {(const void*)k_broaden<true, true>, (const void*)k_broaden<false, true>}, &shm));
    dim3 grid(a.rows, a.B);
    if (shm) {
        hipLaunchKernelGGL((k_broaden<FWD, true>), grid, dim3(256), shm, s, a.in, a.spec, a.rows, a.nf, a.tw,
                           a.dv, a.kind, a.params, a.pstride, a.poff, a.scalar_param, a.out, a.ob, a.orow,
                           a.oelem, (double2*)nullptr, a.info);
    } else {
        hipLaunchKernelGGL((k_broaden<FWD, false>), grid, dim3(256), 0, s, a.in, a.spec, a.rows, a.nf, a.tw,
                           a.dv, a.kind, a.params, a.pstride, a.poff, a.scalar_param, a.out, a.ob, a.orow,
                           a.oelem, a.gscratch, a.info);
    }
    SF_LAUNCH_CHECK();
    return SF_OK;
}

// Hot-path variant (precomputed half spectra): the kernel multiplier depends on the walker only, so it is
// tabulated once per walker (k_kernel_mult) instead of once per row, and the real inverse transform runs
// as a HALF-size complex FFT:  Z_k = (X_k + conj X_{L-k}) + i e^{+2 pi i k/nf} (X_k - conj X_{L-k}),
// L = nf/2;  z = IDFT_L(Z)  =>  x_{2m} = Re z_m, x_{2m+1} = Im z_m.  64 KiB of LDS at nf = 8192.
__global__ __launch_bounds__(256) void k_kernel_mult(double* __restrict__ mult, int nh1, double val, int kind,
                                                     const double* __restrict__ params, int pstride, int poff,
                                                     double scalar_param, int* __restrict__ info) {
    const int b = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
    double param = scalar_param;
    if (params) param = params[(int64_t)b * pstride + poff];
    if (kind == 1 && !(param > 0.0)) {  // transforms.py:121-122
        if (k == 0 && info) atomicCAS(&info[b], 0, SF_INFO_BAD_VSINI);
        return;
    }
    if (k >= nh1) return;
    double m = 1.0;
    if (kind == 1) m = sf_rot_mult(k, val, param);
    else if (kind == 2) m = sf_inst_mult(k, val, param);
    mult[(int64_t)b * nh1 + k] = m;
}

template <bool USE_LDS>
__global__ __launch_bounds__(256) void k_broaden_half(const double2* __restrict__ spec,
                                                      const double* __restrict__ mult, int rows, int nf,
                                                      const double2* __restrict__ tw, int kind,
                                                      const double* __restrict__ params, int pstride, int poff,
                                                      double scalar_param, double* __restrict__ out, int64_t ob,
                                                      int64_t orow, int64_t oelem, double2* __restrict__ gscratch) {
    extern __shared__ __attribute__((aligned(16))) double2 lbuf[];
    const int row = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int L = nf / 2;
    double2* buf = USE_LDS ? lbuf : gscratch + ((int64_t)b * rows + row) * nf;
    double param = scalar_param;
    if (params) param = params[(int64_t)b * pstride + poff];
    if (kind == 1 && !(param > 0.0)) return;  // flagged by k_kernel_mult
    const int bits = sf_log2(L);
    const double2* X = spec + (int64_t)row * (L + 1);
    const double* mb = mult + (int64_t)b * (L + 1);
    for (int k = tid; k < L; k += 256) {
        double2 a = X[k], c = X[L - k];
        const double ma = mb[k], mc = mb[L - k];
        a.x *= ma;
        a.y *= ma;
        c.x *= mc;
        c.y *= mc;
        if (k == 0) a.y = 0.0, c.y = 0.0;  // c2r ignores the imaginary part of DC / Nyquist
        // conj(X_{L-k}) = (c.x, -c.y)
        const double2 E = make_double2(a.x + c.x, a.y - c.y);
        const double2 D = make_double2(a.x - c.x, a.y + c.y);
        const double2 w = tw[k];  // exp(-2 pi i k / nf); we need its conjugate
        const double2 O = make_double2(w.x * D.x + w.y * D.y, w.x * D.y - w.y * D.x);
        buf[sf_bitrev((unsigned)k, bits)] = make_double2(E.x - O.y, E.y + O.x);
    }
    __syncthreads();
    sf_fft_inplace_r4(buf, L, tw, true, 2);
    const double inv_n = 1.0 / nf;
    double* o = out + (int64_t)b * ob + (int64_t)row * orow;
    if (oelem == 1) {  // contiguous row: one 16-byte store per thread
        double2* o2 = (double2*)o;
        for (int m = tid; m < L; m += 256) {
            const double2 z = buf[m];
            o2[m] = make_double2(z.x * inv_n, z.y * inv_n);
        }
    } else {
        for (int m = tid; m < L; m += 256) {
            const double2 z = buf[m];
            o[(int64_t)(2 * m) * oelem] = z.x * inv_n;
            o[(int64_t)(2 * m + 1) * oelem] = z.y * inv_n;
        }
    }
}

// the rows' launch of the hot path: a.mult holds the walkers' multiplier tables
static int launch_broaden_half_rows(const sf_broaden_args& a, hipStream_t s) {
    static sf_dev_once attr_once;  // devices whose function attributes are set
    size_t shm;
    SF_CHECK(sf_fft_place("broaden", a.nf / 2, a.nf, a.gscratch, &attr_once, {(const void*)k_broaden_half<true>}, &shm));
    dim3 grid(a.rows, a.B);
    if (shm) {
        hipLaunchKernelGGL(k_broaden_half<true>, grid, dim3(256), shm, s, a.spec,
                           a.mult, a.rows, a.nf, a.tw, a.kind, a.params, a.pstride, a.poff, a.scalar_param, a.out,
                           a.ob, a.orow, a.oelem, (double2*)nullptr);
    } else {
        hipLaunchKernelGGL(k_broaden_half<false>, grid, dim3(256), 0, s, a.spec, a.mult, a.rows, a.nf, a.tw, a.kind,
                           a.params, a.pstride, a.poff, a.scalar_param, a.out, a.ob, a.orow, a.oelem, a.gscratch);
    }
    SF_LAUNCH_CHECK();
    return SF_OK;
}
static int launch_broaden_half(const sf_broaden_args& a, hipStream_t s) {
    const int nh1 = a.nf / 2 + 1;
    const double val = 1.0 / (a.nf * a.dv);  // numpy.fft.rfftfreq
    hipLaunchKernelGGL(k_kernel_mult, dim3((nh1 + 255) / 256, a.B), dim3(256), 0, s, a.mult, nh1, val, a.kind,
                       a.params, a.pstride, a.poff, a.scalar_param, a.info);
    SF_LAUNCH_CHECK();
    return launch_broaden_half_rows(a, s);
}

int sf_launch_broaden(const sf_broaden_args& a, hipStream_t s) {
    if (a.nf < 4 || (a.nf & (a.nf - 1)) || a.nf > 65536) {
        sf_set_error("broaden: nf=%d must be a power of two in [4, 65536]", a.nf);
        return SF_EINVAL;
    }
    if (!a.in && a.mult) return launch_broaden_half(a, s);
    return a.in ? launch_broaden_t<true>(a, s) : launch_broaden_t<false>(a, s);
}

// Forward half spectrum of static rows (context creation): spec[row][k], k <= nf/2.
template <bool USE_LDS>
__global__ __launch_bounds__(256) void k_rfft_rows(const double* __restrict__ in, int nf,
                                                   const double2* __restrict__ tw,
                                                   double2* __restrict__ spec,
                                                   double2* __restrict__ gscratch) {
    extern __shared__ __attribute__((aligned(16))) double2 lbuf[];
    const int row = blockIdx.x, tid = threadIdx.x;
    double2* buf = USE_LDS ? lbuf : gscratch + (int64_t)row * nf;
    const int bits = sf_log2(nf);
    const double* x = in + (int64_t)row * nf;
    for (int j = tid; j < nf; j += 256) buf[sf_bitrev(j, bits)] = make_double2(x[j], 0.0);
    __syncthreads();
    sf_fft_inplace(buf, nf, tw, false);
    for (int k = tid; k <= nf / 2; k += 256) spec[(int64_t)row * (nf / 2 + 1) + k] = buf[k];
}

int sf_launch_rfft_rows(const double* in, int rows, int nf, const double2* tw, double2* spec,
                        double2* gscratch, hipStream_t s) {
    static sf_dev_once attr_once;  // devices whose function attributes are set
    size_t shm;
    SF_CHECK(sf_fft_place("rfft_rows", nf, nf, gscratch, &attr_once, {(const void*)k_rfft_rows<true>}, &shm));
    if (shm) {
        hipLaunchKernelGGL(k_rfft_rows<true>, dim3(rows), dim3(256), shm, s, in, nf, tw,
                           spec, (double2*)nullptr);
    } else {
        hipLaunchKernelGGL(k_rfft_rows<false>, dim3(rows), dim3(256), 0, s, in, nf, tw, spec, gscratch);
    }
    SF_LAUNCH_CHECK();
    return SF_OK;
}
