// Tile layer of the covariance fill: the 32 x 32 wave sub-tile (rank-m sum on the matrix cores, then everything else),
// the 64 x 64 tile of a workgroup, the tile map of the factorisation and the fill of the likelihood path.
#pragma once

#define FT 64  // tile edge per workgroup (4 waves, 32 x 32 each)

// First half of a tile: the rank-m term of the wave's 32 x 32 sub-tile at (R0, C0) of walker slice Yb, summed over k in
// steps of 4 on v_mfma_f64_16x16x4_f64.  acc[ti][tj] element r = (row R0+ti*16+gam, column C0+tj*16+4q+r).  The ONE
// rolled form (k_fill_dense_plain preloads its fragments instead: the same MFMA sequence per accumulator, the same bits).
__device__ __forceinline__ void sf_rank_m_subtile(const sf_fill_args& a, const double* __restrict__ Yb, int R0, int C0,
                                                  sf_d4 (&acc)[2][2]) {
    const int lane = threadIdx.x & 63;
    const int gam = lane & 15, q = lane >> 4;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (sf_d4){0.0, 0.0, 0.0, 0.0};
    const int colperm = 4 * (gam & 3) + (gam >> 2);
    for (int kk = 0; kk < a.mpad; kk += 4) {
        const double* yk = Yb + (int64_t)(kk + q) * a.ldy;
        double brow[2], acol[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            brow[i] = yk[R0 + i * 16 + gam];
            acol[i] = yk[C0 + i * 16 + colperm];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(acol[j], brow[i], acc[i][j], 0, 0, 0);
    }
}

// Every stored tile in ONE pass: rank-m term on MFMA + sigma^2 on the diagonal + identity padding, and
// (BAND) in the 32 x 32 sub-tiles that intersect the support of a structured kernel: + K_global, then
// + (0 + K_local,0 + K_local,1 ...), then the jitter -- the reference's order of additions
// (spectrum_model.py:338, 348, 353-363, 399).  Write-only: the pass is HBM-write bound (a separate band
// pass used to read-modify-write the same tiles: 1.15 -> 0.5 ms at cfg 2).
// Second half of a tile: the accumulators hold the rank-m term of the wave's 32 x 32 sub-tile at (R0, C0).
template <bool BAND>
__device__ __forceinline__ void sf_tile_finish(const sf_fill_args& a, int b, int R0, int C0, const sf_d4 (&acc)[2][2],
                                               bool mirror = false) {
    const int lane = threadIdx.x & 63;
    const int gam = lane & 15, q = lane >> 4;
    const int nout = sf_fill_extent(a);
    double* __restrict__ Cb = a.C + (int64_t)b * a.stride;
    // which structured kernels reach this 32 x 32 sub-tile (wave-uniform)
    bool do_glob = false;
    sf_global_hyper g = {0, 1, 0};
    unsigned lmask = 0;
    const double* __restrict__ P = a.params + (int64_t)b * a.pstride;
    if (BAND && R0 < a.n && C0 < a.n) {
        if (a.has_global) g = sf_load_global(a, P);
        sf_block_support(a, P, R0, min(R0 + 31, a.n - 1), C0, min(C0 + 31, a.n - 1), g.r0, do_glob, lmask);
    }
    const bool structured = do_glob || lmask;

    const bool vec_ok = ((a.lda | a.stride) & 1) == 0;  // 16-byte stores need even row and matrix strides
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) {
        const int row = R0 + ti * 16 + gam;
        if (row >= nout) continue;
        const double w_row = (BAND && row < a.n) ? a.wave[row] : 1.0;
#pragma unroll
        for (int tj = 0; tj < 2; ++tj) {
            const int col0 = C0 + tj * 16 + 4 * q;
            if (col0 >= nout) continue;
            double v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int col = col0 + r;
                double val = acc[ti][tj][r];
                if (row < a.n && col < a.n) {
                    if (row == col) {
                        const double sg = a.sigma[row];
                        val = val + sg * sg;                                     // spectrum_model.py:338
                    }
                } else {
                    val = (row == col) ? 1.0 : 0.0;  // identity padding up to the Cholesky leaf
                }
                v[r] = val;
            }
            if (BAND && structured && row < a.n) {
                double w_col[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) w_col[r] = (col0 + r < a.n) ? a.wave[col0 + r] : 1.0;
                if (do_glob && a.gtab) {  // log-uniform grid: one value per diagonal (see k_band_gtab)
                    const double* gt = a.gtab + (int64_t)b * a.n;
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (col0 + r < a.n) v[r] = v[r] + gt[abs(row - (col0 + r))];
                } else if (do_glob) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (col0 + r < a.n) v[r] = v[r] + sf_matern_elem(w_row, w_col[r], g.amp, g.ls, g.r0);
                }
                if (lmask) {
                    double loc[4] = {0.0, 0.0, 0.0, 0.0};
                    for (int k = 0; k < a.n_local; ++k) {
                        if (!((lmask >> k) & 1)) continue;
                        const sf_local_hyper l = sf_load_local(a, P, k);
                        const double d_row = sf_local_metric(w_row, l.mu);
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            loc[r] = loc[r] + sf_local_elem(d_row, sf_local_metric(w_col[r], l.mu), l.amp, l.sig, 4 * l.sig);
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (col0 + r < a.n) v[r] = v[r] + loc[r];
                }
            }
            if (a.add_jitter && row < a.n) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (col0 + r == row) v[r] = v[r] + SF_JITTER;  // spectrum_model.py:399
            }
            double* dst = Cb + (int64_t)row * a.lda + col0;
            if (vec_ok && col0 + 3 < nout) {
                *(double2*)dst = make_double2(v[0], v[1]);
                *(double2*)(dst + 2) = make_double2(v[2], v[3]);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (col0 + r < nout) dst[r] = v[r];
            }
            if (mirror) {
                // C is symmetric bit for bit (every term's formula is symmetric in (row, column), the MFMA sums over k in
                // the same order): the dense fill evaluates the structured tiles below the diagonal only and writes
                // each one a second time transposed -- 16 lanes cover 128 contiguous bytes of a row of the mirror tile
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (col0 + r < nout) Cb[(int64_t)(col0 + r) * a.lda + row] = v[r];
            }
        }
    }
}

template <bool BAND>
__device__ __forceinline__ void sf_fill_tile(const sf_fill_args& a, int b, int tm, int tn) {
    if (a.lower_only && tn > tm) return;
    if (a.tilemap) {  // (tm, tn) count 64-row tiles of the MATRIX; the map is indexed in the factorisation's frame
        const int fs = a.fp >> 6;
        if (!a.tilemap[(int64_t)b * a.nt128 * a.nt128 + ((tm + fs) >> 1) * a.nt128 + ((tn + fs) >> 1)]) return;
    }

    const int w = threadIdx.x >> 6;
    const int R0 = tm * FT + (w >> 1) * 32, C0 = tn * FT + (w & 1) * 32;
    const int nout = sf_fill_extent(a);  // extent of the stored matrix
    if (R0 >= nout || C0 >= nout) return;
    if (a.lower_only && C0 > R0 + 31) return;
    const double* __restrict__ Yb = a.Y + (int64_t)b * a.mpad * a.ldy;
    sf_d4 acc[2][2];
    sf_rank_m_subtile(a, Yb, R0, C0, acc);
    sf_tile_finish<BAND>(a, b, R0, C0, acc);
}

// Which 128 x 128 tiles of the lower triangle carry anything besides the rank-m term (diagonal
// SF_NB blocks: sigma^2 / jitter / identity padding; Matern band; local patches)?  Only those are
// materialised for the factorisation; the MFMA update kernel generates the others from Y on the fly.
__global__ __launch_bounds__(256) void k_tile_map(sf_fill_args a) {
    const int nt = a.nt128;
    const int e = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (e >= nt * nt) return;
    const int tm = e / nt, tn = e - tm * nt;
    unsigned char flag = 0;
    if (tn <= tm) {
        // tile (tm, tn) of the factorisation's frame = rows 128 tm - fp .. of the matrix (a.fp leading virtual rows)
        const int vr = tm * 128, vc = tn * 128;
        const int rlo = max(vr - a.fp, 0), clo = max(vc - a.fp, 0);
        if (vr / SF_NB == vc / SF_NB || rlo >= a.n) {
            flag = 1;  // diagonal block (or pure padding rows)
        } else {  // strictly below the diagonal: the same test as the sub-tiles of the tile, or the fill would drop covariance
            const int rhi = min(vr - a.fp + 127, a.n - 1), chi = min(vc - a.fp + 127, a.n - 1);
            const double* __restrict__ P = a.params + (int64_t)b * a.pstride;
            bool do_glob;
            unsigned lmask;
            sf_block_support(a, P, rlo, rhi, clo, chi, a.has_global ? sf_load_global(a, P).r0 : 0.0, do_glob, lmask);
            flag = (do_glob || lmask) ? 1 : 0;
        }
    }
    a.tilemap[(int64_t)b * nt * nt + e] = flag;
    if (flag && a.tilelist) {
        const int idx = atomicAdd(&a.tilecount[b], 1);  // (the order of the list does not matter: tiles are independent)
        if (idx < a.list_cap) a.tilelist[(int64_t)b * a.list_cap + idx] = ((unsigned)tm << 16) | (unsigned)tn;
    }
}

template <bool BAND>
__global__ __launch_bounds__(256, BAND ? 2 : 4) void k_fill_tiles(sf_fill_args a, int nt) {
    const int id = sf_xcd_remap(blockIdx.x, gridDim.x);
    const int tiles = nt * nt;
    const int b = id / tiles;
    const int t = id - b * tiles;
    sf_fill_tile<BAND>(a, b, t / nt, t - (t / nt) * nt);
}
// The likelihood path: G workgroups per walker walk the walker's list of materialised 128 x 128 tiles (four 64 x 64 tiles
// each).  The one-workgroup-per-tile grid above is 524 288 workgroups at cfg 2 of which nine in ten leave at once:
// dispatch-bound (0.70 ms for 0.9 GB written).
template <bool BAND>
__global__ __launch_bounds__(256, BAND ? 2 : 4) void k_fill_tiles_list(sf_fill_args a, int G) {
    const int b = blockIdx.x / G, g = blockIdx.x - b * G;
    const int cnt = min(a.tilecount[b], a.list_cap) * 4;
    const unsigned* __restrict__ list = a.tilelist + (int64_t)b * a.list_cap;
    const int fs = a.fp >> 6;  // the list holds tiles of the factorisation's frame: a.fp / 64 virtual 64-row tiles in front
    for (int li = g; li < cnt; li += G) {
        const unsigned e = list[li >> 2];
        const int tm = 2 * (int)(e >> 16) + ((li >> 1) & 1) - fs, tn = 2 * (int)(e & 0xffff) + (li & 1) - fs;
        if (tm >= 0 && tn >= 0) sf_fill_tile<BAND>(a, b, tm, tn);
    }
}

int sf_launch_fill(const sf_fill_args& a, int B, hipStream_t s) {
    SF_CHECK(sf_check_n_local(a));
    if (a.fp != 0 && (a.fp != 64 || !a.tilemap || !a.lower_only)) {
        sf_set_error("fill: a shifted tile frame needs fp = 64, a tile map and lower_only");
        return SF_EINVAL;
    }
    const int nout = sf_fill_extent(a);
    const int nt = (nout + FT - 1) / FT;
    const long long nblk = (long long)nt * nt * B;
    SF_CHECK(sf_check_fill_grid(nblk));
    const bool listed = a.tilemap && a.tilelist && a.tilecount && a.lower_only;
    if (a.tilemap) {
        if (listed) SF_HIP(hipMemsetAsync(a.tilecount, 0, sizeof(int) * (size_t)B, s));
        hipLaunchKernelGGL(k_tile_map, dim3((a.nt128 * a.nt128 + 255) / 256, B), dim3(256), 0, s, a);
        SF_LAUNCH_CHECK();
    }
    const int structured = a.has_global || a.n_local > 0;
    sf_fill_args a2 = a;
    if (!(a.gtab && a.has_global && a.loguniform && a.lower_only)) a2.gtab = nullptr;
    if (a2.gtab) {
        hipLaunchKernelGGL(k_band_gtab, dim3((a.n + 255) / 256, B), dim3(256), 0, s, a, a2.gtab, a.n - 1);
        SF_LAUNCH_CHECK();
    }
    if (listed) {
        const int G = 64;
        if (structured) hipLaunchKernelGGL(k_fill_tiles_list<true>, dim3((unsigned)B * G), dim3(256), 0, s, a2, G);
        else hipLaunchKernelGGL(k_fill_tiles_list<false>, dim3((unsigned)B * G), dim3(256), 0, s, a2, G);
    } else if (structured) hipLaunchKernelGGL(k_fill_tiles<true>, dim3((unsigned)nblk), dim3(256), 0, s, a2, nt);
    else hipLaunchKernelGGL(k_fill_tiles<false>, dim3((unsigned)nblk), dim3(256), 0, s, a2, nt);
    SF_LAUNCH_CHECK();
    return SF_OK;
}
