// The diagonal 128 x 128 tile resident in LDS: sf_diag_lds_body, its kernel k_diag_lds and sf_launch_diag128.
// Used by the fused, wide and band sequences (the launch) and by the diagonal-tile tasks of k_potrf_dataflow (the body).
#pragma once
#include "sf_device.h"
#include "sf_chol_tile.h"

// The same diagonal-block step for the 128-column panels of the fused sequence, with the tile and its growing inverse
// RESIDENT IN LDS: k_diag_mfma keeps them in the L2-backed scratch, so every one of its 8 block columns pays two global
// round trips (stage L(k,:), write X / read it back as an operand of the next column), 55-65 us per tile when the chip
// is idle and three times that beside the panel launches.  Here the tile is read once, the eight columns run out of LDS
// (no staging buffers: an accumulator block is written to its own destination block and read back in operand layout
// by the same wave), and L / L^-1 / z are written once.
// The inverse grows IN PLACE of the factor (36 blocks of 16 x 17 doubles + one: 79.6 KB, two workgroups per CU or one
// beside a panel workgroup; with a second set of blocks for the inverse it was 157 KB = a whole CU): block column k of
// W = L^-T is row k of L^-1, and row k of L is read for the last time at step k -- by the waves that update block column
// k and by the waves that accumulate row k of the inverse, all before that step's first barrier -- so after it the
// inverse waves drop X(e, k) into the slot of L(k, e).  L leaves for global memory block by block as it becomes final.
// (body shared by the kernel below and by the diagonal-tile tasks of k_potrf_dataflow; dsm: SF_DIAG_LDS_BYTES of LDS)
#ifdef SF_TUNING
#define SF_D_STAMP(i) do { if (stamps && tid == 0) stamps[i] = wall_clock64(); } while (0)
#else
#define SF_D_STAMP(i)
#endif
__device__ __forceinline__ void sf_diag_lds_body(const double* __restrict__ T, int64_t sT, int pw, int* __restrict__ info,
                                                 int info_off, double* __restrict__ rhs, int ldr,
                                                 double* __restrict__ Cdiag, int ldc, int64_t sC,
                                                 double* __restrict__ Wt, int64_t sW, int fp0, const int b,
                                                 double* __restrict__ dsm, const int tid, long long* stamps = nullptr) {
    SF_D_STAMP(0);
    // fp0: the first fp0 rows / columns of the tile are virtual (identity in T; Cdiag and rhs point fp0 elements BEFORE
    // the matrix there: never stored, read as zero) -- the first tile of a shifted frame, see sf_potrf_front_pad
    double* Tl = dsm;              // lower blocks (bi >= bj) of the tile at (bi (bi + 1) / 2 + bj) * DBS
    double* El = Tl;               // blocks X(e, j), e <= j, of W = L_kk^-T: in the slot of L(j, e) once row j of L is dead
    double* Fb = Tl + 36 * DBS;    // inverse of the current 16 x 16 diagonal factor
    double* rz = Fb + DBS;         // [128]
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lq = lane >> 4;
    const int nb = pw >> 4;
    const double* Tb = T + (int64_t)b * sT;
    double* Cb = Cdiag + (int64_t)b * sC;
    double* Wb = Wt + (int64_t)b * sW;
    auto tb = [](int bi, int bj) { return (bi * (bi + 1) / 2 + bj) * DBS; };
    auto eb = [](int e, int j) { return (j * (j + 1) / 2 + e) * DBS; };  // = tb(j, e)

    {
        // the lower blocks only, 16 bytes per load, ALL of a thread's loads in flight before the first LDS store (nine per
        // thread for a full tile: one round trip instead of thirty-two short ones; 5.5 -> ~3 us of the tile's 41)
        const int cnt = nb * (nb + 1) / 2 * 128;
        double2 v[9];
#pragma unroll
        for (int u = 0; u < 9; ++u) {
            const int e = min(tid + 512 * u, cnt - 1);
            const int blk = e >> 7, r = (e >> 3) & 15, c2 = e & 7;
            int bi = 0;
            while ((bi + 1) * (bi + 2) / 2 <= blk) ++bi;
            const int bj = blk - bi * (bi + 1) / 2;
            v[u] = *(const double2*)(Tb + (int64_t)(16 * bi + r) * SF_LDT + 16 * bj + 2 * c2);
        }
#pragma unroll
        for (int u = 0; u < 9; ++u) {
            const int e = tid + 512 * u;
            if (e < cnt) {
                const int r = (e >> 3) & 15, c2 = e & 7;
                double* d = Tl + (e >> 7) * DBS + r * DLD + 2 * c2;  // (tb(bi, bj) = blk * DBS: the same enumeration)
                d[0] = v[u].x;
                d[1] = v[u].y;
            }
        }
    }
    __syncthreads();
    SF_D_STAMP(1);
    int bad = 0;
    const int oF = l15 * DLD + lq;  // operand fragment: row l15, K slice lq of instruction kk stands for k = 4 kk + lq
    for (int k = 0; k < nb; ++k) {
        const int m = nb - 1 - k;
        if (k == 7) SF_D_STAMP(8);
        // ---- U: wave t <= m holds M(k + t, k), wave t > m the block X(t - m - 1, k) of the inverse
        const int t = wave;
        const bool has = t <= m + k, isM = t <= m;
        const int ib = isM ? k + t : t - m - 1;
        double* own = has ? (isM ? Tl + tb(ib, k) : El + eb(ib, k)) : Fb;
        sf_d4 acc = {0.0, 0.0, 0.0, 0.0};
        if (has) {
            if (isM) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = lq + 4 * r;  // (the diagonal block is read symmetrically from its lower triangle)
                    acc[r] = t == 0 ? own[max(row, l15) * DLD + min(row, l15)] : own[row * DLD + l15];
                }
            }
            for (int j = isM ? 0 : ib; j < k; ++j) {
                const double* ap = (isM ? Tl + tb(ib, j) : El + eb(ib, j)) + oF;
                const double* bp = Tl + tb(k, j) + oF;
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ap[4 * kk], bp[4 * kk], acc, 0, 0, 1);  // neg:[1,0,0]
            }
        }
        // ---- P: wave 0 factorises the diagonal block and inverts the factor in the accumulator layout
        if (k == 7) SF_D_STAMP(9);
        if (wave == 0) {
            sf_d4 a0 = acc, f, lt;
            double pkeep;
            SF_POTRF16_ACC(a0, lane, l15, lq, f, lt, pkeep);
            const unsigned long long neg = __ballot(lane < 16 && !(pkeep > 0.0));
            if (neg && !bad) bad = 16 * k + __ffsll((long long)neg);
            double* Ekk = El + eb(k, k);  // (= own: the diagonal block of the tile has been consumed)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = lq + 4 * r;
                Fb[row * DLD + l15] = f[r];
                Ekk[l15 * DLD + row] = f[r];                      // X of the identity row block k is F^T
                // L[i][j], lower triangle of the diagonal block: straight to the matrix
                if (l15 >= row && 16 * k + row >= fp0) Cb[(int64_t)(16 * k + l15) * ldc + 16 * k + row] = lt[r];
            }
        }
        if (k == 7) SF_D_STAMP(10);
        __syncthreads();
        if (k == 7) SF_D_STAMP(11);
        // ---- X: the other blocks times F^T, through their own destination block (accumulator -> operand layout)
        if (has && wave != 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) own[(lq + 4 * r) * DLD + l15] = acc[r];
            double a[4], f4[4];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                a[kk] = own[oF + 4 * kk];
                f4[kk] = Fb[oF + 4 * kk];
            }
            sf_d4 x = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) x = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk], f4[kk], x, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) own[(lq + 4 * r) * DLD + l15] = x[r];
            if (isM && 16 * k + l15 >= fp0) {  // block (k + t, k) of L is final
#pragma unroll
                for (int r = 0; r < 4; ++r) Cb[(int64_t)(16 * ib + lq + 4 * r) * ldc + 16 * k + l15] = x[r];
            }
        }
        __syncthreads();
    }
    SF_D_STAMP(2);
    if (tid == 0 && bad && info && info[b] == 0) info[b] = info_off + bad;
    // ---- Wt[c][j] = (L_kk^-1)[c][j] (block (cb, jb) = X(jb, cb)^T, zero above)
    for (int idx = tid; idx < nb * nb * 128; idx += 512) {  // (16-byte stores: half as many store instructions per thread)
        const int blk = idx >> 7, bi = blk / nb, bj = blk - bi * nb, r = (idx >> 3) & 15, c = (idx & 7) * 2;
        const double* e = El + eb(bj, bi) + c * DLD + r;
        *(double2*)(Wb + (int64_t)(16 * bi + r) * SF_LDT + 16 * bj + c) = bj <= bi ? make_double2(e[0], e[DLD]) : make_double2(0.0, 0.0);
    }
    // ---- z_k = L_kk^-1 r_k with the explicit inverse
    if (rhs) {
        double* rb = rhs + (int64_t)b * ldr;
        if (tid < pw) rz[tid] = tid >= fp0 ? rb[tid] : 0.0;
        __syncthreads();
        {
            // four lanes per row (j = p, p + 4, ... <= i each), added by two shuffles: the 128-term chain of one lane per row
            // was 3.9 us of the tile's 41
            const int i = tid >> 2, p = tid & 3, ibk = i >> 4, ir = i & 15;
            double zacc = 0.0;
            if (i < pw)
                for (int j = p; j <= i; j += 4) zacc = __builtin_fma(El[eb(j >> 4, ibk) + (j & 15) * DLD + ir], rz[j], zacc);
            zacc += __shfl_xor(zacc, 1);
            zacc += __shfl_xor(zacc, 2);
            if (p == 0 && i < pw && i >= fp0) rb[i] = zacc;
        }
    }
#ifdef SF_TUNING
    if (stamps) {
        SF_D_STAMP(3);
        __syncthreads();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        SF_D_STAMP(4);
    }
#endif
}
__global__ __launch_bounds__(512) void k_diag_lds(const double* __restrict__ T, int64_t sT, int pw, int* __restrict__ info,
                                                  int info_off, double* __restrict__ rhs, int ldr,
                                                  double* __restrict__ Cdiag, int ldc, int64_t sC,
                                                  double* __restrict__ Wt, int64_t sW, int fp0, int prio, long long* stamps) {
    extern __shared__ double dsm[];
    if (prio) __builtin_amdgcn_s_setprio(2);
    sf_diag_lds_body(T, sT, pw, info, info_off, rhs, ldr, Cdiag, ldc, sC, Wt, sW, fp0, blockIdx.x, dsm, threadIdx.x,
                     blockIdx.x == 0 ? stamps : nullptr);
}
#define SF_DIAG_LDS_BYTES ((37 * DBS + 128) * sizeof(double))
// (the chain's workgroups -- this launch and the narrow steps that park the next diagonal tile -- run at raised wave priority)
static int sf_launch_diag128(double* T, int64_t sT, int pw, int* info, int info_off, double* rhs, int ldr, double* Cdiag,
                             int ldc, int64_t sC, double* Wt, int64_t sW, int batch, hipStream_t s, int fp0 = 0) {
    static sf_dev_once attr_once;  // devices whose function attributes are set
    SF_CHECK(sf_lds_limit_once(&attr_once, 160 * 1024, {(const void*)k_diag_lds}));
    long long* stamps = nullptr;
#ifdef SF_TUNING
    static int printed = 0;
    static long long* hs = nullptr;
    if (SF_TUNE_FLAG("SF_DIAG_STAMPS") && printed < 6) {
        if (!hs) SF_HIP(hipHostMalloc((void**)&hs, 16 * sizeof(long long)));
        for (int i = 0; i < 16; ++i) hs[i] = 0;
        stamps = hs;
    }
#endif
    hipLaunchKernelGGL(k_diag_lds, dim3(batch), dim3(512), SF_DIAG_LDS_BYTES, s, T, sT, pw, info, info_off, rhs, ldr, Cdiag, ldc,
                       sC, Wt, sW, fp0, 1, stamps);
#ifdef SF_TUNING
    if (stamps) {  // (synchronises) phases of workgroup 0, us
        (void)hipStreamSynchronize(s);
        ++printed;
        fprintf(stderr, "k_diag_lds batch %d: tile load %.1f | 8 block columns %.1f (last column: U %.1f, P %.1f, barrier %.1f, X + barrier %.1f) | W store %.1f + z %.1f | drain %.1f | total %.1f us\n",
                batch, (hs[1] - hs[0]) / 100.0, (hs[2] - hs[1]) / 100.0, (hs[9] - hs[8]) / 100.0, (hs[10] - hs[9]) / 100.0, (hs[11] - hs[10]) / 100.0,
                (hs[2] - hs[11]) / 100.0, 0.0, (hs[3] - hs[2]) / 100.0, (hs[4] - hs[3]) / 100.0, (hs[4] - hs[0]) / 100.0);
    }
#endif
    SF_LAUNCH_CHECK();
    return SF_OK;
}
#undef SF_D_STAMP
