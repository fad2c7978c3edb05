// Shape of the band solver's LDS window (sf_band.hip), stated once for the kernel, its launchers, the workspace layout and
// the CPU check (tests/hostmath_driver.cpp, command `band`).  Plain C++, no HIP header: the functions are host + device
// under hipcc and plain inline functions under the host compiler.
#pragma once
#include <stddef.h>

#ifdef __HIPCC__
#define SFB_HD __host__ __device__ inline
#else
#define SFB_HD inline
#endif

#define BB 16
#define BS (BB * (BB + 1))  // doubles per stored block (row stride 17: conflict-free fragment reads)
#define BLD (BB + 1)
#define SFB_PF 4            // prefetch registers per thread
#define SFB_PT 8            // update pairs per wave (table row; the last entry is the count)
#define SFB_LDS_MAX (160 * 1024)             // dynamic LDS one workgroup may ask for
#define SF_BAND_TILES_MAX_HALFWIDTH 768      // wide bands (beyond the window): bordered band matrices, sf_launch_potrf_band

SFB_HD int sfb_nbr(int halfwidth) {  // window blocks per side: window rows >= W + 16, and at least three blocks
    const int nbr = (halfwidth + 2 * BB - 1) / BB;
    return nbr < 3 ? 3 : nbr;
}
SFB_HD int sfb_nrb(int nrhs) { return (nrhs + BB - 1) / BB; }  // 16-row blocks of right-hand sides
#define SFB_MIX_MAX_ROWS 48  // right-hand sides of a sweep in all: three blocks (sfb_admit)
// Waves 4.. prefetch the band rows in groups of 256 threads (one 16 x 16 block per group and register): enough groups
// for SFB_PF registers to cover the nbr blocks of a block row
SFB_HD int sfb_nwaves(int nbr) { return nbr <= SFB_PF ? 8 : nbr <= 2 * SFB_PF ? 12 : 16; }
SFB_HD int sfb_loader_groups(int nwaves) { return (nwaves - 4) >> 2; }  // 256-thread groups of band loaders (1..3)

// The dynamic LDS of k_band_forms<NRB>, regions in this order; offsets in doubles (the integer regions start on doubles too):
//   Wb    nbr (nbr + 1) / 2 band blocks             RH   [nrb][nbr] right-hand-side blocks (column ring)
//   Fb2   [2] inverse of the diagonal factor, L_kk^-1 (by parity of k)   G   [NR][NR + 1] Gram accumulator, NR = 16 nrb
//   pv    [2][16] pivots (for the log-determinant)  red  [16] reduction scratch
//   sync  16 ints: progress flags of the pipeline   ptab [16 waves][SFB_PT] ints: update pairs
//   reserve  64 bytes nothing uses: the launch has always asked for them
struct sfb_lds {
    int Wb, RH, Fb2, G, pv, red, sync, ptab, reserve, doubles;
    size_t bytes;
};
SFB_HD sfb_lds sfb_lds_layout(int nbr, int nrb) {
    const int NR = nrb * BB;
    sfb_lds L;
    L.Wb = 0, L.RH = L.Wb + (nbr * (nbr + 1) / 2) * BS, L.Fb2 = L.RH + nrb * nbr * BS, L.G = L.Fb2 + 2 * BS;
    L.pv = L.G + NR * (NR + 1), L.red = L.pv + 2 * BB, L.sync = L.red + BB, L.ptab = L.sync + 16 / 2;
    L.reserve = L.ptab + 16 * SFB_PT / 2, L.doubles = L.reserve + 8;
    L.bytes = sizeof(double) * (size_t)L.doubles;
    return L;
}

// Which solver takes a half-width with nrhs right-hand sides: the LDS window (k_band_forms), the bordered band matrices
// on the tile kernels (sf_launch_potrf_band), or neither.  The ONE place that compares against the LDS limit.
enum sfb_path { SFB_NEITHER = 0, SFB_WINDOW, SFB_TILES };
SFB_HD sfb_path sfb_admit(int halfwidth, int nrhs) {
    const int nrb = sfb_nrb(nrhs);
    if (halfwidth < 0 || nrhs < 1 || nrb > 3) return SFB_NEITHER;  // (three blocks of right-hand sides on either path)
    if (sfb_lds_layout(sfb_nbr(halfwidth), nrb).bytes <= SFB_LDS_MAX) return SFB_WINDOW;
    return halfwidth <= SF_BAND_TILES_MAX_HALFWIDTH ? SFB_TILES : SFB_NEITHER;
}
SFB_HD int sf_band_max_halfwidth(int nrhs) {  // largest half-width the window takes (a multiple of 16); -1: none
    int best = -1;
    for (int w = 0; sfb_admit(w, nrhs) == SFB_WINDOW; w += BB) best = w;
    return best;
}

// Position of a wave among the workers (waves 1..), those on wave 0's SIMD last; -1 for wave 0
SFB_HD int sfb_worker_pos(int wave, int nwaves) {
    const int nprim = nwaves - (nwaves >> 2);  // workers that do not share wave 0's SIMD
    return wave == 0 ? -1 : (wave & 3) ? wave - 1 - (wave >> 2) : nprim + (wave >> 2) - 1;
}
// Update pairs of the RB (RB + 1) / 2 block pairs (I >= J) of a column dealt to that worker: round robin from pair 1 on
// (pair 0 is wave 0's), the remainder to the first positions
SFB_HD int sfb_worker_pairs(int wpos, int nworkers, int RB) {
    const int npairs = RB * (RB + 1) / 2, first = 1 + wpos;
    return first < npairs ? (npairs - first + nworkers - 1) / nworkers : 0;
}

// Two-sided ("twisted") sweep over nblk block columns: the top-down half eliminates the first kend0, the bottom-up half
// the last kend1; both stop at the separator of nm rows (nbr - 1 blocks)
struct sfb_twist {
    int nm, kend0, kend1;
};
SFB_HD sfb_twist sfb_twist_shape(int nblk, int nbr) {
    const int kend0 = (nblk - (nbr - 1)) / 2;
    return sfb_twist{(nbr - 1) * BB, kend0, nblk - (nbr - 1) - kend0};
}
SFB_HD bool sfb_twist_fits(int nblk, int nbr) { return nblk >= 2 * nbr + (nbr - 1); }  // each half sweeps at least a window
// Its workspace, carved from `base` (null: only counted, as the layouts of sf_work.h)
//   dumpM [batch][2][nm * nm]  what each half leaves of the separator block     dumpR [batch][2][NR * nm]  ... of the right-hand-
//   side rows over the separator columns     dumpG [batch][2][nrhs * nrhs], dumpL [batch][2]  partial Gram matrices, log-determinants
//   mband [batch][nm * nm]  merged separator in band storage     mrhs [batch][NR * nm]  its right-hand sides
//   gadd [batch][nrhs * nrhs], ladd [batch]  sums of the partial Gram matrices and log-determinants
struct sfb_twist_work {
    double *dumpM, *dumpR, *dumpG, *dumpL, *mband, *mrhs, *gadd, *ladd;
    size_t doubles;
};
inline sfb_twist_work sfb_twist_carve(double* base, int halfwidth, int nrhs, int batch) {
    const size_t nm = (size_t)(sfb_nbr(halfwidth) - 1) * BB, NR = (size_t)sfb_nrb(nrhs) * BB, ng = (size_t)nrhs * nrhs, b = (size_t)batch;
    size_t off = 0;
    auto take = [&](size_t count) {
        off += count;
        return base ? base + (off - count) : nullptr;
    };
    sfb_twist_work w;
    w.dumpM = take(2 * b * nm * nm), w.dumpR = take(2 * b * NR * nm), w.dumpG = take(2 * b * ng), w.dumpL = take(2 * b);
    w.mband = take(b * nm * nm), w.mrhs = take(b * NR * nm), w.gadd = take(b * ng), w.ladd = take(b);
    w.doubles = off + 64;  // (slack the size has always included)
    return w;
}

// Whether two half sweeps per matrix pay.  One workgroup occupies a CU for the whole sweep, so the launch takes
// ceil(workgroups / CUs) rounds.  Two half sweeps per matrix are half as long each but twice as many, plus merge and
// separator sweep (measured ~12 % of a sweep per round of matrices): take them when that means less time -- batch <=
// CUs/2, and again wherever the last round of single sweeps would be mostly empty (CUs < batch <= 1.5 CUs, ...).
// Measured at cfg 2: B = 300: 2.37 -> 1.96 ms, 384: 2.34 -> 1.98, 640: 3.55 -> 3.25; B = 1600 (cfg 3 shape) stays with
// single sweeps (6.13 vs 6.39 ms).
SFB_HD bool sfb_twist_pays(int nblk, int nbr, int batch, int ncu) {
    if (nblk < 6 * nbr) return false;
    const int rounds1 = (batch + ncu - 1) / ncu, rounds2 = (2 * batch + ncu - 1) / ncu;
    return 0.5 * rounds2 + 0.12 * rounds1 < (double)rounds1;
}

// ---- the full solve x = A^-1 rhs (sf_band_solve.h): what the keeping sweep stores, and the backward sweep's LDS
// Per block column k the keeping sweep writes one record of nbr + nrb row-major 16 x 16 blocks (no row padding):
//   [0] F_k = L_kk^-1    [1 + I] L_{k+1+I,k}, I < nbr - 1    [nbr + rb] block rb of the forward-substituted right-hand
//   sides (L^-1 rhs)_k, transposed: rows = right-hand sides, columns = the 16 pixels of the column
SFB_HD int sfb_keep_column_blocks(int nbr, int nrb) { return nbr + nrb; }
SFB_HD size_t sfb_keep_block(int kb, int j, int nbr, int nrb) {  // offset of block j of column kb's record, in doubles
    return ((size_t)kb * sfb_keep_column_blocks(nbr, nrb) + j) * (BB * BB);
}
SFB_HD size_t sfb_keep_doubles(int n, int nbr, int nrb) {  // stored factor + right-hand sides of one matrix: ~ n (W + 16 + nrhs)
    return sfb_keep_block((n + BB - 1) / BB, 0, nbr, nrb);
}
// The backward sweep k_band_back<NRB>: SFB_BACK_SPLIT waves per block of right-hand sides share the sum over a column's
// blocks.  Its dynamic LDS, offsets in doubles (blocks of BS doubles, row stride 17):
//   T     [nrb][nbr] ring of the solved blocks, slot = block column % nbr
//   part  [nrb][SFB_BACK_SPLIT] partial sums of the step
#define SFB_BACK_SPLIT 4
struct sfb_back_lds {
    int T, part, doubles;
    size_t bytes;
};
SFB_HD sfb_back_lds sfb_back_lds_layout(int nbr, int nrb) {
    sfb_back_lds L;
    L.T = 0, L.part = L.T + nrb * nbr * BS, L.doubles = L.part + nrb * SFB_BACK_SPLIT * BS;
    L.bytes = sizeof(double) * (size_t)L.doubles;
    return L;
}
SFB_HD int sfb_back_nwaves(int nrb) { return SFB_BACK_SPLIT * nrb; }
SFB_HD int sfb_back_blocks_per_wave(int nbr) { return (nbr - 1 + SFB_BACK_SPLIT - 1) / SFB_BACK_SPLIT; }  // factor blocks a wave holds
#define SFB_BACK_MAX_BLOCKS 3  // ... at the widest window the LDS admits (nbr = 10)

// ---- selected inversion (sf_band_selinv.h): the band of Sigma = A^-1 from the kept factor, block columns from the last to
// the first.  k_band_selinv runs one wave per block below the diagonal of a block column (nbr - 1 waves).  Its dynamic LDS,
// offsets in doubles (blocks of BS doubles, row stride 17):
//   S  nbr (nbr + 1) / 2 blocks of Sigma, the lower triangle of the window, addressed by the unordered pair of ring slots
//      {row block % nbr, column block % nbr} as the forward sweep's window (the full square does not fit: the upper half is
//      read transposed)
//   G  [nbr - 1] the step's G_I = L_{k+1+I,k} F_k          P  [nbr - 1] the step's products G_I^T Sigma_{k+1+I,k}
// 158848 bytes at nbr = 10: every half-width the window admits with one block of right-hand sides (144) fits.
struct sfb_selinv_lds {
    int S, G, P, doubles;
    size_t bytes;
};
SFB_HD sfb_selinv_lds sfb_selinv_lds_layout(int nbr) {
    sfb_selinv_lds L;
    L.S = 0, L.G = L.S + (nbr * (nbr + 1) / 2) * BS, L.P = L.G + (nbr - 1) * BS, L.doubles = L.P + (nbr - 1) * BS;
    L.bytes = sizeof(double) * (size_t)L.doubles;
    return L;
}
SFB_HD int sfb_selinv_nwaves(int nbr) { return nbr - 1; }
#define SFB_SELINV_MAX_WAVES 9  // ... at nbr = 10
SFB_HD bool sfb_selinv_admits(int halfwidth) {  // every half-width of the window: sfb_admit(halfwidth, 1) == SFB_WINDOW
    return sfb_admit(halfwidth, 1) == SFB_WINDOW && sfb_selinv_lds_layout(sfb_nbr(halfwidth)).bytes <= SFB_LDS_MAX &&
           sfb_selinv_nwaves(sfb_nbr(halfwidth)) <= SFB_SELINV_MAX_WAVES;
}
