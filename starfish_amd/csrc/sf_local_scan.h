// The score (Lagrange-multiplier) scan for a NEW local kernel of centre mu and width sigma at amplitude 0, given everything that
// is already in C: with k = the fill's local element at amplitude 1 (sf_local_elem on sf_local_metric, cut-off 4 sigma),
//     quad = alpha^T k alpha,   trace = tr(W k),   fisher = 1/2 tr(W k W k),      alpha = C^-1 r,  W = C^-1,
// so that d lnL / dA at A = 0 is 1/2 (quad - trace) and fisher its information.  k lives on the pixels within 4 sigma of mu, on
// a monotonic grid a contiguous patch [lo, hi]: all three numbers need alpha and W on the patch only.  A layer of sf_fill.hip
// behind the gradient's head (the factor, X = L^-1):
//
//   k_ls_wband   once per walker: the 64 x 64 tiles (I, J) of W with 0 <= I - J <= reach (sf_cinv_tile), each stored with its
//                mirror image: wband[b][A][K - A + reach] is the tile (rows of block A, columns of block K), row-major, for
//                |A - K| <= reach -- either orientation is read k-contiguously.  reach = min(SF_LS_REACH, blocks - 1): the blocks
//                a patch of SF_LS_MAXP pixels can span beyond its first.  Nothing else of W is formed.
//   k_ls_patch   one workgroup per candidate: [lo, hi] = the pixels with sf_local_metric <= 4 sigma (1 + 1e-9), the margin of
//                sf_block_support.  (0, -1): no pixel in reach; a candidate that is no kernel (mu or sigma not positive and
//                finite) or whose patch is wider than the launcher's limit (max_patch: SF_LS_MAXP here, less on the band solver,
//                sf_band_local_scan.h) is marked wider than SF_LS_MAXP.
//   k_ls_cand    one 4-wave workgroup per (walker, candidate), over the blocks Ib0 = lo / 64 .. Ib1 = hi / 64 of the patch.  Per
//                pair (I, J <= I), ascending: M = sum_K W_IK k_KJ and N = sum_K k_IK W_KJ (= the transpose of sum_K W_JK k_KI)
//                on v_mfma_f64_16x16x4_f64 through sf_inv_sweep, K ascending; the tiles of k are generated into LDS from the
//                element formulas (rows and columns outside [lo, hi]: zero by mask, nothing is evaluated for them), k_JK as the
//                columns of k_KJ, k_IK as the rows.  The pair adds sum_ab M_ab N_ab to fisher and, from the tile k_IJ in LDS, sum_ab
//                alpha_a alpha_b k_ab to quad and sum_ab W_ab k_ab to trace, each times sf_grad_weight.  A thread sums its 16
//                entries of a pair, then the pairs in order; the wave's sum (xor shuffles) and the four waves in wave order follow.
//                No M goes to global memory.
// A candidate's numbers depend on nothing but its walker and (mu, sigma): not on the other candidates, the batch or the chunk.
// No pixel in reach: exactly 0, 0, 0.  A patch wider than SF_LS_MAXP pixels: NaN, NaN, NaN for every walker.  info != 0: NaN,
// nothing of the walker is read.  No atomics, no workgroup waits for another, every sum in a fixed order.
#pragma once

#define SF_LS_REACH ((SF_LS_MAXP + SF_LEAF - 2) / SF_LEAF)  // blocks beyond its first that such a patch can span (4)
#define SF_LS_LDD 66    // row stride of the tile of k in LDS (SF_FC_LDD)

struct sf_ls_args {
    sf_fill_args f;       // wave, n and the factored matrices as sf_launch_cov_grad gets them (C: L below, X^T above)
    const double* winv;   // [batch][npad / 64][64][64]
    const double* alpha;  // [batch][ld_alpha]
    int ld_alpha;
    const int* info;      // [batch]
    const double* cand;   // [ncand][2]: mu, sigma
    int ncand, batch, nbr, reach;
    int* patch;           // [ncand][2]: lo, hi
    double* wband;        // [batch][nbr][2 reach + 1][64][64]
    double* out;          // [batch][ncand][3]
    int max_patch;        // widest patch in pixels that k_ls_patch lets through (<= SF_LS_MAXP; the last field: k_ls_cand's offsets stay)
};
size_t sf_local_scan_band_doubles(int n, int batch) {
    const size_t nbr = (size_t)(n + SF_LEAF - 1) / SF_LEAF;
    const size_t reach = nbr - 1 < SF_LS_REACH ? nbr - 1 : SF_LS_REACH;
    return (size_t)batch * nbr * (2 * reach + 1) * (SF_LEAF * SF_LEAF);
}
// the tile (rows of block A, columns of block K) of walker b's band, |A - K| <= reach
__device__ __forceinline__ double* sf_ls_tile(const sf_ls_args& a, int b, int A, int K) {
    return a.wband + (((int64_t)b * a.nbr + A) * (2 * a.reach + 1) + (K - A + a.reach)) * (SF_LEAF * SF_LEAF);
}

__global__ __launch_bounds__(256) void k_ls_wband(const sf_ls_args a) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, lq = lane >> 4;
    const int b = blockIdx.x % a.batch, id = blockIdx.x / a.batch;
    const int I = id / (a.reach + 1), J = I - id % (a.reach + 1);
    if (J < 0 || a.info[b] != 0) return;
    const sf_fill_args& f = a.f;
    sf_d4 acc[4];
    sf_cinv_tile(sf_cinv_source(f.C, f.npad, f.lda, f.stride, a.winv, b), I, J, w, l15, lq, acc);
    sf_fc_store(acc, sf_ls_tile(a, b, I, J), SF_LEAF, w, l15, lq);
    if (J < I) {  // the mirror image: (column, row)
        double* dst = sf_ls_tile(a, b, J, I);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) dst[(16 * t + l15) * SF_LEAF + 16 * w + lq + 4 * r] = acc[t][r];
    }
}

__global__ __launch_bounds__(256) void k_ls_patch(const sf_ls_args a) {
    __shared__ int s_lo[4], s_hi[4];
    const int tid = threadIdx.x, q = blockIdx.x, n = a.f.n;
    const double mu = a.cand[2 * q], sg = a.cand[2 * q + 1];
    const bool kernel = mu > 0.0 && sg > 0.0 && mu < __builtin_inf() && sg < __builtin_inf();
    int lo = n, hi = -1;
    if (kernel) {
        const double r0 = 4 * sg;
        for (int i = tid; i < n; i += 256)
            if (sf_local_metric(a.f.wave[i], mu) <= r0 * (1 + 1e-9)) lo = min(lo, i), hi = max(hi, i);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) lo = min(lo, __shfl_xor(lo, off)), hi = max(hi, __shfl_xor(hi, off));
    if ((tid & 63) == 0) s_lo[tid >> 6] = lo, s_hi[tid >> 6] = hi;
    __syncthreads();
    if (tid == 0) {
        lo = min(min(s_lo[0], s_lo[1]), min(s_lo[2], s_lo[3]));
        hi = max(max(s_hi[0], s_hi[1]), max(s_hi[2], s_hi[3]));
        if (!kernel || hi - lo + 1 > a.max_patch) lo = 0, hi = SF_LS_MAXP;  // (wider than the limit: NaN)
        else if (hi < 0) lo = 0;
        a.patch[2 * q] = lo, a.patch[2 * q + 1] = hi;
    }
}

__global__ __launch_bounds__(256) void k_ls_cand(const sf_ls_args a) {
    __shared__ double s_k[64 * SF_LS_LDD];
    __shared__ double s_met[(SF_LS_REACH + 1) * SF_LEAF];  // the metric of the pixels of the patch's blocks
    __shared__ double s_red[12];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, lq = lane >> 4;
    const int q = blockIdx.x, b = blockIdx.y;
    double* out = a.out + ((int64_t)b * a.ncand + q) * 3;
    const int lo = a.patch[2 * q], hi = a.patch[2 * q + 1];
    const bool wide = hi - lo + 1 > SF_LS_MAXP;
    if (wide || a.info[b] != 0 || hi < lo) {  // (the same in every thread)
        if (tid < 3) out[tid] = (wide || a.info[b] != 0) ? __builtin_nan("") : 0.0;
        return;
    }
    const double mu = a.cand[2 * q], sg = a.cand[2 * q + 1], r0 = 4 * sg;
    const int Ib0 = lo >> 6, Ib1 = hi >> 6, P0 = Ib0 * SF_LEAF;  // (Ib1 - Ib0 <= reach: hi - lo < SF_LS_MAXP, hi < n)
    for (int i = tid; i < (Ib1 - Ib0 + 1) * SF_LEAF; i += 256) {
        const int p = P0 + i;
        s_met[i] = p >= lo && p <= hi ? sf_local_metric(a.f.wave[p], mu) : -1.0;  // (-1: outside the patch)
    }
    const double* al = a.alpha + (int64_t)b * a.ld_alpha;
    const int k = tid & 63, c0 = tid >> 6;  // this thread generates column k of the rows c0 + 4 e of a tile
    // s_k[c][k] = k(pixel 64 R + c, pixel 64 K + k)
    auto generate = [&](int R, int K) {
        const double d_k = s_met[(K - Ib0) * SF_LEAF + k];
#pragma unroll 4
        for (int e = 0; e < 16; ++e) {
            const int c = c0 + 4 * e;
            const double d_c = s_met[(R - Ib0) * SF_LEAF + c];
            double v = 0.0;
            if (d_k >= 0.0 && d_c >= 0.0) v = sf_local_elem(d_c, d_k, 1.0, sg, r0);
            s_k[c * SF_LS_LDD + k] = v;
        }
    };
    const double* krow = s_k + (16 * w + l15) * SF_LS_LDD;
    const double* kcol[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) kcol[t] = s_k + (16 * t + l15) * SF_LS_LDD;
    double vq = 0.0, vt = 0.0, vf = 0.0;
    for (int I = Ib0; I <= Ib1; ++I) {
        double a_r[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = I * SF_LEAF + 16 * w + lq + 4 * r;
            a_r[r] = i >= lo && i <= hi ? al[i] : 0.0;
        }
        for (int J = Ib0; J <= I; ++J) {
            sf_d4 M[4], N[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) M[t] = N[t] = sf_d4{0.0, 0.0, 0.0, 0.0};
            double pq = 0.0, pt = 0.0;
            for (int K = Ib0; K <= Ib1; ++K) {
                __syncthreads();  // s_met is written; the last tile is read
                generate(J, K);
                __syncthreads();
                // M += W_IK k_KJ: column c of k_KJ is row c of k_JK
                sf_inv_sweep(sf_ls_tile(a, b, I, K) + (16 * w + l15) * SF_LEAF, true, kcol, true, 0, SF_LEAF, lq, M);
                if (J != I) {  // (the same in every thread)
                    __syncthreads();
                    generate(I, K);
                    __syncthreads();
                }
                // N += k_IK W_KJ: column c of W_KJ is row c of W_JK
                const double* wc[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) wc[t] = sf_ls_tile(a, b, J, K) + (16 * t + l15) * SF_LEAF;
                sf_inv_sweep(krow, true, wc, true, 0, SF_LEAF, lq, N);
                if (K == J) {  // s_k holds k_IJ: the pair's part of quad and trace
                    const double* Wt = sf_ls_tile(a, b, I, J);
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int j = J * SF_LEAF + 16 * t + l15;
                        const double a_c = j >= lo && j <= hi ? al[j] : 0.0;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = 16 * w + lq + 4 * r;
                            const double kv = s_k[row * SF_LS_LDD + 16 * t + l15];
                            pq = pq + a_r[r] * a_c * kv;
                            pt = pt + Wt[row * SF_LEAF + 16 * t + l15] * kv;
                        }
                    }
                }
            }
            double pf = 0.0;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) pf = pf + M[t][r] * N[t][r];
            const double wgt = sf_grad_weight(I, J);
            vq = vq + wgt * pq, vt = vt + wgt * pt, vf = vf + wgt * pf;
        }
    }
    vq = sf_wave_sum(vq), vt = sf_wave_sum(vt), vf = sf_wave_sum(vf);
    if (lane == 0) s_red[3 * w] = vq, s_red[3 * w + 1] = vt, s_red[3 * w + 2] = vf;
    __syncthreads();
    if (tid < 3) {
        const double s = ((s_red[tid] + s_red[3 + tid]) + s_red[6 + tid]) + s_red[9 + tid];
        out[tid] = tid == 2 ? 0.5 * s : s;
    }
}

// the launches behind the inverse: the band of W, the patches, the candidates
int sf_launch_local_scan(const sf_fill_args& f, int batch, const double* winv, const double* alpha, int ld_alpha, const int* info,
                         const double* cand, int ncand, int* patch, double* wband, double* out, hipStream_t s) {
    sf_ls_args a;
    a.f = f;
    a.winv = winv, a.alpha = alpha, a.ld_alpha = ld_alpha, a.info = info, a.cand = cand, a.ncand = ncand, a.batch = batch;
    a.nbr = (f.n + SF_LEAF - 1) / SF_LEAF, a.reach = a.nbr - 1 < SF_LS_REACH ? a.nbr - 1 : SF_LS_REACH;
    a.patch = patch, a.wband = wband, a.out = out;
    a.max_patch = SF_LS_MAXP;
    if (f.n <= 0 || !f.monotonic || f.npad % SF_LEAF != 0 || f.npad < a.nbr * SF_LEAF || ld_alpha < f.n || batch < 1 ||
        batch > 65535 || ncand < 1 || ncand > 65535) {
        sf_set_error("local scan: n > 0 on a monotonic grid, npad a multiple of %d, batch and ncand in 1 .. 65535", SF_LEAF);
        return SF_EINVAL;
    }
    const long long tiles = (long long)batch * a.nbr * (a.reach + 1);
    SF_CHECK(sf_check_fill_grid(tiles));
    hipLaunchKernelGGL(k_ls_wband, dim3((unsigned)tiles), dim3(256), 0, s, a);
    SF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ls_patch, dim3(ncand), dim3(256), 0, s, a);
    SF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ls_cand, dim3(ncand, batch), dim3(256), 0, s, a);
    SF_LAUNCH_CHECK();
    return SF_OK;
}
