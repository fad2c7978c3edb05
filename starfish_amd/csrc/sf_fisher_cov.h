// The Fisher information of the covariance hyper-parameters,
//     F_ij = 1/2 tr(C^-1 dC_i C^-1 dC_j) = 1/2 sum_ab (dC_i)_ab (S_j)_ab,   S_j = W dC_j W,  W = C^-1,
// in the slots of sf_cov_grad.h (log_amp, log_ls of the global kernel, then mu, log_amp, log_sigma per local kernel).  A layer of
// sf_fill.hip behind the gradient's head (the factor, X = L^-1): the entry derivatives, the support test and the block-row
// contraction frame are the gradient's; the two products that turn dC_j into S_j are this layer's.  One slot j at a time:
//
//   k_fc_winv      once per walker: every 64 x 64 tile of W (sf_cinv_tile) for J <= I, stored with its mirror image in a dense
//                  symmetric matrix wf[b][ldw][ldw], ldw = 64 ceil(n / 64) (sf_fisher_cov_ld).
//   k_fc_left      T_j = W dC_j, one workgroup per SF_FC_IB tiles (I .. I + 3, J) of the column blocks J that slot j's kernel
//                  reaches (sf_fc_reach of (J, J)): over the K with (K, J) reached, in ascending order, the derivative tile is
//                  generated into LDS from the entry formulas (rows and columns >= n: zero), transposed so that both MFMA
//                  operands are k-contiguous, and multiplied on v_mfma_f64_16x16x4_f64 with the rows of W of every block row
//                  read as sf_inv_sweep reads them.
//   k_fc_contract  the gradient's block-row kernel (k_cov_grad) with the tile alpha alpha^T - G replaced by the tile of
//                  S_j = T_j W: per supported pair (I, J <= I) that a slot i >= j reaches, the tile is the sweep of the rows of
//                  T_j against the rows of W (= its columns) over the column blocks T_j has, in ascending order, and is
//                  contracted with the derivative entries of the slots i >= j's components as k_cov_grad contracts its tile.
//   k_fc_sum       one thread per (walker, i >= j) adds the block rows in ascending order, times 1/2, and writes F_ij and its
//                  mirror F_ji (the same bits); NaN where info != 0.
// Nothing of a walker with info != 0 is read.  No atomics, no workgroup waits for another, every sum in a fixed order that
// does not depend on the batch.  Rows and columns >= n: their derivative entries are zero by mask, nothing is written for
// them beyond the tiles of wf and T_j, which are scratch.
#pragma once

#define SF_FC_LDD 66       // row stride of the derivative tile in LDS: rows 16-byte aligned, 16 rows on 16 distinct slots
#define SF_FC_MAXB 1024    // block rows whose reach flags a workgroup holds (n <= 65536)
#define SF_FC_IB 4         // block rows of T_j one workgroup of k_fc_left forms from one generated derivative tile

// slot j -> its component and which derivative of it
struct sf_fc_slot {
    int comp;   // -1: the global kernel; c >= 0: local kernel c
    int which;  // global: 0 log_amp, 1 log_ls; local: 0 mu, 1 log_amp, 2 log_sigma
    sf_global_hyper g;
    sf_local_hyper l;
};
__device__ __forceinline__ sf_fc_slot sf_fc_slot_of(const sf_fill_args& f, const double* __restrict__ P, int j) {
    sf_fc_slot s;
    s.g = sf_global_hyper{0, 1, 0};
    s.l = sf_local_hyper{1, 0, 1};
    const int gslots = f.has_global ? 2 : 0;
    if (f.has_global) s.g = sf_load_global(f, P);
    if (j < gslots) {
        s.comp = -1, s.which = j;
    } else {
        s.comp = (j - gslots) / 3, s.which = (j - gslots) % 3;
        s.l = sf_load_local(f, P, s.comp);
    }
    return s;
}
// (dC_j)_(row, col) from the wavelengths of the two pixels
__device__ __forceinline__ double sf_fc_entry(const sf_fc_slot& s, double w_row, double w_col) {
    if (s.comp < 0) {
        double k, k_ls;
        sf_matern_grad_elem(w_row, w_col, s.g, k, k_ls);
        return s.which == 0 ? k : k_ls;
    }
    double k, k_mu, k_sig;
    sf_local_grad_elem(sf_local_metric(w_row, s.l.mu), sf_local_metric_dmu(w_row, s.l.mu), sf_local_metric(w_col, s.l.mu),
                       sf_local_metric_dmu(w_col, s.l.mu), s.l, k, k_mu, k_sig);
    return s.which == 0 ? k_mu : (s.which == 1 ? k : k_sig);
}
// does the component of slot s reach block (A, B) (either order: the test is symmetric)?
__device__ __forceinline__ bool sf_fc_reach(const sf_fill_args& f, const double* __restrict__ P, const sf_fc_slot& s, int A, int B) {
    bool dg;
    unsigned lm;
    const int n = f.n;
    sf_block_support(f, P, A * 64, min(A * 64 + 63, n - 1), B * 64, min(B * 64 + 63, n - 1), s.g.r0, dg, lm);
    return s.comp < 0 ? dg : ((lm >> s.comp) & 1u) != 0;
}

struct sf_fc_args {
    sf_fill_args f;      // wave, params and the model's layout as the fill gets them (C: the factored matrices, X^T above)
    const double* winv;  // [batch][npad / 64][64][64]
    double* wf;          // [batch][ldw][ldw]: W, both triangles
    double* tj;          // [batch][ldw][ldw]: T_j, the column blocks slot j reaches
    int ldw, slot;
    sf_grad_out o;       // part: [batch][nbr][nslots] (of slot j: the entries i >= j); grad: d_fisher, grad_stride: of a matrix
};

// store the accumulator tile (register r of acc[t] = (row 16 w + lq + 4 r, column 16 t + l15)) at dst, row stride ld
__device__ __forceinline__ void sf_fc_store(const sf_d4 (&acc)[4], double* dst, int ld, int w, int l15, int lq) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) dst[(int64_t)(16 * w + lq + 4 * r) * ld + 16 * t + l15] = acc[t][r];
}

__global__ __launch_bounds__(256) void k_fc_winv(const sf_fc_args a) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, lq = lane >> 4;
    const int b = blockIdx.x % a.o.batch, ij = blockIdx.x / a.o.batch;
    const int I = ij / a.o.nbr, J = ij % a.o.nbr;
    if (J > I || a.o.info[b] != 0) return;
    const sf_fill_args& f = a.f;
    sf_d4 acc[4];
    sf_cinv_tile(sf_cinv_source(f.C, f.npad, f.lda, f.stride, a.winv, b), I, J, w, l15, lq, acc);
    double* Wb = a.wf + (int64_t)b * a.ldw * a.ldw;
    sf_fc_store(acc, Wb + (int64_t)I * 64 * a.ldw + J * 64, a.ldw, w, l15, lq);
    if (J < I) {  // the mirror image: (column, row)
        double* dst = Wb + (int64_t)J * 64 * a.ldw + I * 64;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) dst[(int64_t)(16 * t + l15) * a.ldw + 16 * w + lq + 4 * r] = acc[t][r];
    }
}

__global__ __launch_bounds__(256) void k_fc_left(const sf_fc_args a) {
    __shared__ double s_d[64 * SF_FC_LDD];  // [column of block J][row k of block K]
    __shared__ unsigned char s_reach[SF_FC_MAXB];
    const sf_fill_args& f = a.f;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, lq = lane >> 4;
    const int n = f.n, nbr = a.o.nbr;
    const int b = blockIdx.x % a.o.batch, ij = blockIdx.x / a.o.batch;
    const int I0 = (ij / nbr) * SF_FC_IB, J = ij % nbr;
    if (a.o.info[b] != 0) return;
    const double* __restrict__ P = f.params + (int64_t)b * f.pstride;
    const sf_fc_slot sl = sf_fc_slot_of(f, P, a.slot);
    if (!sf_fc_reach(f, P, sl, J, J)) return;  // (the same in every thread) T_j has no such column block: k_fc_contract skips it
    for (int K = tid; K < nbr; K += 256) s_reach[K] = sf_fc_reach(f, P, sl, K, J) ? 1 : 0;
    const double* Wb = a.wf + (int64_t)b * a.ldw * a.ldw;
    const double* arow = Wb + (int64_t)(I0 * 64 + 16 * w + l15) * a.ldw;
    const double* bc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) bc[t] = s_d + (16 * t + l15) * SF_FC_LDD;
    sf_d4 acc[SF_FC_IB][4];
#pragma unroll
    for (int ii = 0; ii < SF_FC_IB; ++ii)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[ii][t] = sf_d4{0.0, 0.0, 0.0, 0.0};
    const int k = tid & 63, c0 = tid >> 6;  // this thread generates row k of block K against columns c0 + 4 e of block J
    for (int K = 0; K < nbr; ++K) {
        __syncthreads();  // s_reach is written; the last tile is read
        if (!s_reach[K]) continue;
        const int row = K * 64 + k;
        const bool ok_row = row < n;
        const double w_row = ok_row ? f.wave[row] : 1.0;
#pragma unroll 4
        for (int e = 0; e < 16; ++e) {
            const int c = c0 + 4 * e, col = J * 64 + c;
            double v = 0.0;
            if (ok_row && col < n) v = sf_fc_entry(sl, w_row, f.wave[col]);
            s_d[c * SF_FC_LDD + k] = v;
        }
        __syncthreads();
#pragma unroll
        for (int ii = 0; ii < SF_FC_IB; ++ii)
            if (I0 + ii < nbr) sf_inv_sweep(arow + (int64_t)ii * 64 * a.ldw + K * 64, true, bc, true, 0, 64, lq, acc[ii]);
    }
    double* Tb = a.tj + (int64_t)b * a.ldw * a.ldw;
#pragma unroll
    for (int ii = 0; ii < SF_FC_IB; ++ii)
        if (I0 + ii < nbr) sf_fc_store(acc[ii], Tb + (int64_t)(I0 + ii) * 64 * a.ldw + J * 64, a.ldw, w, l15, lq);
}

__global__ __launch_bounds__(256) void k_fc_contract(const sf_fc_args a) {
    __shared__ unsigned s_lmask[SF_GRAD_SB];
    __shared__ unsigned char s_glob[SF_GRAD_SB];
    __shared__ unsigned char s_has[SF_FC_MAXB];  // column blocks of T_j
    __shared__ double s_sum[2 + 3 * SF_MAX_LOCAL];
    __shared__ double s_red[12];
    const sf_fill_args& f = a.f;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, lq = lane >> 4;
    const int n = f.n, nbr = a.o.nbr;
    int b, I;
    if (!sf_grad_block(a.o, b, I)) return;
    const double* __restrict__ P = f.params + (int64_t)b * f.pstride;
    const sf_fc_slot sl = sf_fc_slot_of(f, P, a.slot);
    const sf_global_hyper gh = sl.g;
    const int gslots = f.has_global ? 2 : 0;
    const int c_first = sl.comp < 0 ? 0 : sl.comp;      // the local components of the slots i >= j
    const unsigned lwant = ~0u << c_first;
    const bool gwant = sl.comp < 0;                    // the global kernel's slots are among them
    for (int q = tid; q < a.o.nslots; q += 256) s_sum[q] = 0.0;
    for (int L = tid; L < nbr; L += 256) s_has[L] = sf_fc_reach(f, P, sl, L, L) ? 1 : 0;
    const double* Wb = a.wf + (int64_t)b * a.ldw * a.ldw;
    const double* trow = a.tj + (int64_t)b * a.ldw * a.ldw + (int64_t)(I * 64 + 16 * w + l15) * a.ldw;
    const int R0 = I * 64, rhi = min(R0 + 63, n - 1);
    double w_r[4];  // wavelength of this thread's rows
    bool ok_r[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = R0 + 16 * w + lq + 4 * r;
        ok_r[r] = i < n;
        w_r[r] = ok_r[r] ? f.wave[i] : 1.0;
    }
    for (int sb0 = 0; sb0 <= I; sb0 += SF_GRAD_SB) {
        const int nsb = min(SF_GRAD_SB, I + 1 - sb0);
        __syncthreads();  // the flags of the last chunk are read; s_sum is zeroed, s_has written
        if (tid < nsb) {
            const int clo = (sb0 + tid) * 64;
            bool dg;
            unsigned lm;
            sf_block_support(f, P, R0, rhi, clo, min(clo + 63, n - 1), gh.r0, dg, lm);
            s_glob[tid] = dg && gwant ? 1 : 0;
            s_lmask[tid] = lm & lwant;
        }
        __syncthreads();
        for (int jj = 0; jj < nsb; ++jj) {
            const bool dg = s_glob[jj] != 0;
            const unsigned lm = s_lmask[jj];
            if (!dg && !lm) continue;  // (the same in every thread)
            const int J = sb0 + jj, C0 = J * 64;
            const double wgt = sf_grad_weight(I, J);
            // the tile of S_j = T_j W: rows of T_j against rows of W (W is symmetric), over the column blocks T_j has
            sf_d4 A[4];
            const double* wc[4];
            double w_c[4];
            bool ok_c[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                A[t] = sf_d4{0.0, 0.0, 0.0, 0.0};
                wc[t] = Wb + (int64_t)(C0 + 16 * t + l15) * a.ldw;
                ok_c[t] = C0 + 16 * t + l15 < n;
                w_c[t] = ok_c[t] ? f.wave[C0 + 16 * t + l15] : 1.0;
            }
            for (int L0 = 0; L0 < nbr;) {  // runs of column blocks, ascending
                if (!s_has[L0]) {
                    ++L0;
                    continue;
                }
                int L1 = L0 + 1;
                while (L1 < nbr && s_has[L1]) ++L1;
                sf_inv_sweep(trow, true, wc, true, L0 * 64, L1 * 64, lq, A);
                L0 = L1;
            }
            if (dg) {
                double v[3] = {0.0, 0.0, 0.0};
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if (!(ok_r[r] && ok_c[t])) continue;
                        double k, k_ls;
                        sf_matern_grad_elem(w_r[r], w_c[t], gh, k, k_ls);
                        v[0] = v[0] + A[t][r] * k;
                        v[1] = v[1] + A[t][r] * k_ls;
                    }
                sf_cov_grad_flush(v, 2, wgt, s_red, s_sum, tid);
            }
            for (int c = c_first; c < f.n_local; ++c) {
                if (!((lm >> c) & 1u)) continue;
                const sf_local_hyper l = sf_load_local(f, P, c);
                double d_r[4], dp_r[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    d_r[r] = sf_local_metric(w_r[r], l.mu);
                    dp_r[r] = sf_local_metric_dmu(w_r[r], l.mu);
                }
                double v[3] = {0.0, 0.0, 0.0};
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const double d_c = sf_local_metric(w_c[t], l.mu), dp_c = sf_local_metric_dmu(w_c[t], l.mu);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if (!(ok_r[r] && ok_c[t])) continue;
                        double k, k_mu, k_sig;
                        sf_local_grad_elem(d_r[r], dp_r[r], d_c, dp_c, l, k, k_mu, k_sig);
                        v[0] = v[0] + A[t][r] * k_mu;
                        v[1] = v[1] + A[t][r] * k;
                        v[2] = v[2] + A[t][r] * k_sig;
                    }
                }
                sf_cov_grad_flush(v, 3, wgt, s_red, s_sum + gslots + 3 * c, tid);
            }
        }
    }
    __syncthreads();
    double* part = sf_grad_part(a.o, b, I);
    for (int q = tid; q < a.o.nslots; q += 256) part[q] = s_sum[q];
}

// F_ij for i >= j = a.slot and its mirror
__global__ void k_fc_sum(const sf_fc_args a) {
    const sf_grad_out& o = a.o;
    const int i = a.slot + blockIdx.x * blockDim.x + threadIdx.x, j = a.slot, b = blockIdx.y;
    if (i >= o.nslots) return;
    double s = 0.0;
    if (o.info[b] != 0) {
        s = __builtin_nan("");
    } else {
        for (int I = 0; I < o.nbr; ++I) s = s + o.part[((int64_t)b * o.nbr + I) * o.nslots + i];
        s = 0.5 * s;
    }
    double* F = o.grad + (int64_t)b * o.grad_stride;
    F[i * o.nslots + j] = s;
    F[j * o.nslots + i] = s;
}

int sf_launch_fisher_cov(const sf_fill_args& f, int batch, const double* winv, const int* info, double* wf, double* tj, double* part,
                         double* fisher, int fisher_stride, hipStream_t s) {
    SF_CHECK(sf_check_n_local(f));
    sf_fc_args a;
    a.f = f;
    a.winv = winv, a.wf = wf, a.tj = tj, a.ldw = sf_fisher_cov_ld(f.n), a.slot = 0;
    const int nbr = (f.n + 63) / 64, ns = sf_cov_grad_slots(f.has_global, f.n_local);
    a.o = sf_grad_out{info, part, nbr, ns, batch, fisher, fisher_stride};
    if (f.n <= 0 || f.npad % SF_LEAF != 0 || f.npad < a.ldw || nbr > SF_FC_MAXB || ns < 1 || fisher_stride < ns * ns || batch < 1 ||
        batch > 65535) {
        sf_set_error("cov fisher: 0 < n <= %d, npad a multiple of %d, a structured kernel, fisher_stride >= slots^2, batch in 1 .. 65535",
                     64 * SF_FC_MAXB, SF_LEAF);
        return SF_EINVAL;
    }
    const long long tiles = (long long)batch * nbr * nbr, rows = (long long)batch * nbr;
    const long long left = (long long)batch * ((nbr + SF_FC_IB - 1) / SF_FC_IB) * nbr;
    SF_CHECK(sf_check_fill_grid(tiles));
    hipLaunchKernelGGL(k_fc_winv, dim3((unsigned)tiles), dim3(256), 0, s, a);
    SF_LAUNCH_CHECK();
    for (int j = 0; j < ns; ++j) {
        a.slot = j;
        hipLaunchKernelGGL(k_fc_left, dim3((unsigned)left), dim3(256), 0, s, a);
        SF_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_fc_contract, dim3((unsigned)rows), dim3(256), 0, s, a);
        SF_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_fc_sum, dim3((ns - j + 63) / 64, batch), dim3(64), 0, s, a);
        SF_LAUNCH_CHECK();
    }
    return SF_OK;
}
