// Batched fp64 Cholesky (lower, row-major, in place) + logdet / Mahalanobis solve for gfx950.
//
// Replaces the LAPACK calls of the reference: scipy.linalg.cho_factor / cho_solve at
// Starfish/models/spectrum_model.py:400-404 (dpotrf + dpotrs on the N x N covariance).
//
// One launch sequence serves the whole batch (the batch supplies the parallelism).  sf_potrf_pick chooses among four
// (numbers and measurements: DESIGN.md section 3; sf_debug_cholesky_sequence forces one):
//   4  dataflow: the whole factorisation as ONE persistent launch, k_potrf_dataflow, whose workgroups draw tasks (the
//      bodies of the panel step and of the diagonal tile) ordered by counters -- while batch x panels <= 2048, up to 128
//      matrices and 65 panels, unless the persistent kernel has been switched off.  sf_launch_potrf_v4.
//   2  wide: a PAIR of 128-column panels per launch, k_chol_panel_w (one 16-wave workgroup per CU keeps a 128 x 256
//      tile), with narrow steps for the chain -- from batch x slabs >= 3400 at n >= 2048.  sf_launch_potrf_v3.
//   0  fused: LEFT-looking panels of 128 columns, k_chol_panel -- one workgroup per 128-row slab does the long-K update,
//      the triangular solve against the explicit inverse of the diagonal tile, the in-place store of L, the forward
//      substitution of the right-hand side and the update of its own diagonal tile; k_diag_lds factors the diagonal
//      tile (L_kk, L_kk^-1, z_k) on the side stream; launches that cannot fill the chip are split along K -- every
//      other batch of 16 matrices or more.  sf_launch_potrf_v2.
//   1  unfused (round 1): panels of SF_NB = 256 columns, k_gemm_nt into a panel scratch, k_diag_mfma on 256 x 256
//      blocks, separate solve and diagonal-update launches -- below 16 matrices while the persistent kernel is
//      switched off.  sf_launch_potrf_v1.
// sf_launch_potrf_band runs bordered band matrices on the fused kernels.  k_logdet_z: logdet = 2 sum log L_ii and
// sqmah = |z|^2 (z = L^-1 R is produced inside the factorisation); k_trsv_logdet: the stand-alone forward substitution.
//
// ONE translation unit; layers are headers, included in dependency order (a later one may use an earlier one):
//   sf_device.h          lane / wave helpers, XCD remap, the 16 x 16 factor step (shared with the other .hip files)
//   sf_chol_tile.h       tile constants
//   sf_chol_host.h       scratch layout, split-K policy, frame helpers, fork / join: what every launcher shares
//   sf_chol_unfused.h    everything only sequence 1 uses
//   sf_chol_diag.h       the diagonal tile in LDS: sf_diag_lds_body, k_diag_lds
//   sf_chol_sync.h       counters, waits, watch and rescue of the persistent kernel
//   sf_chol_solve.h      k_logdet_z, k_trsv_logdet, the clock probe
//   sf_chol_apply.h      the factor applied to right-hand sides (L Z, L^-1 B, L^-T B, C^-1 B): k_chol_apply; independent of the sequences
//   sf_chol_inverse.h    diag(C^-1) from the factor, the column norms of L^-1: k_chol_block_inverse, k_chol_inverse_diag; independent of the sequences
//   sf_chol_panel.h      the panel step: sf_panel_args, sf_panel_body, k_chol_panel
//   sf_chol_wide.h       the wide step (a pair of panels): sf_panelw_args, k_chol_panel_w
//   sf_chol_seq.h        the narrow and wide steps as launches, the narrow step of a chain and two slab groups,
//                        sf_launch_potrf_v2 (fused) and sf_launch_potrf_v3 (wide)
//   sf_chol_band.h       the band driver: border / finish kernels, sf_launch_potrf_band
//   sf_chol_dataflow.h   the persistent kernel k_potrf_dataflow, its counters, abort record and enable flag, sf_launch_potrf_v4
// This file itself: which sequence runs, when, and on whose measurement.
#include <atomic>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "sf_common.h"
#include <stdio.h>
#include "sf_device.h"
#include "sf_chol_tile.h"
#include "sf_chol_host.h"
#include "sf_chol_unfused.h"
#include "sf_chol_diag.h"
#include "sf_chol_sync.h"
#include "sf_chol_solve.h"
#include "sf_chol_apply.h"
#include "sf_chol_inverse.h"
#include "sf_chol_panel.h"
#include "sf_chol_wide.h"
#include "sf_chol_seq.h"
#include "sf_chol_band.h"
#include "sf_chol_dataflow.h"

static std::atomic<int> g_chol_sequence{-1};
int sf_set_cholesky_sequence(int mode) {
    if (mode < -1 || mode > 4) {
        sf_set_error("cholesky sequence: -1 automatic, 0 fused panel kernel, 1 unfused, 2 wide (panel pairs), 3 wide then narrow (test aid), 4 dataflow");
        return SF_EINVAL;
    }
    g_chol_sequence.store(mode);
    return SF_OK;
}

// Small batches are bound by the number of sequential long-K steps; the unfused sequence has half as many (256-column
// panels).  Measured at N = 4096, fused (partial sums of top(k) beside D(k), chain at raised wave priority) / unfused:
// B = 12: 10.0 / 9.05-9.6 ms, 16: 10.97 / 11.1, 20: 12.2 / 12.6, 24: 13.3 / 13.9, 32: 15.4 / 16.9, 64: 26.1 / 29.5.
#define SF_UNFUSED_BELOW 16
// The dataflow sequence (one persistent launch) wins wherever the launch sequences cannot keep the chip full between their
// panel boundaries.  Measured (tools/bench_potrf.py, same box, launch sequences (fused; wide where it is their choice) /
// dataflow): N = 4096: B = 8 7.4 / 5.1 ms, 16: 9.6 / 7.85, 32: 14.2 / 13.7, 48: 20.0 / 19.9, 64: 25.9 / 25.45, 80: 31.9 / 32.1,
// 96: 37.5 / 38.3, 112: 42.4 / 44.4, 128: 47.1 / 50.7; N = 3008: B = 16 6.15 / 4.7, 64: 11.8 / 11.5, 96: 16.7 / 16.9; N = 2048:
// B = 16 3.36 / 2.5, 128: 8.15 / 8.1; N = 1024: B = 16 1.29 / 0.88, 256: 2.8 / 3.2 (32 matrices per queue: the dispenser's scan
// of their chain counters shows)  ->  taken while batch x panels <= 2048 and batch <= 128.
static bool sf_potrf_dataflow_auto(int n, int batch) {
    // (round 6: the panel count is the true one -- N = 4096: up to 64 matrices, the half-ensemble of a 128-walker sampler; same
    // box, persistent kernel / fused sequence there: 25.5 / 26.0 ms.  Rounds 4-5 counted 64 virtual rows more: 62 matrices.)
    const int nt = (n + GT - 1) / GT;
    // (... and stops at N = 8192: the kernel FITS up to N = 16384 -- forced sequence 4, tests -- but was only ever measured to
    // win up to 65 panels; at N = 16384 the tasks are milliseconds long and the launch sequences keep the chip as full:
    // profiles/r06_a_dataflow_n16384.txt)
    return sf_potrf_dataflow_fits(n, batch) && (long long)batch * nt <= 2048 && batch <= 128 && nt <= 65;
}
// The sequence that factorises `batch` matrices of order n (the numbering of sf_set_cholesky_sequence): the forced one, or
// the automatic choice.  (A matrix with more panels than the dataflow tables hold takes the fused sequence when the dataflow
// one is forced.)
static int sf_potrf_pick(int n, int batch) {
    const int sel = g_chol_sequence.load();  // sf_debug_cholesky_sequence(): tests drive all five
    if (sel == 4 && !sf_potrf_dataflow_fits(n, batch)) return 0;
    if (sel >= 0) return sel;
    if (sf_potrf_dataflow_auto(n, batch)) return 4;
    // The wide sequence (panel pairs, one 16-wave workgroup per CU) halves the A-operand stream and a third of all HBM
    // traffic of the factorisation, but one workgroup per CU has nothing to overlap its epilogue and barriers with: it pays
    // once its launches are many rounds of workgroups.  Measured (bench.py, same box, fused / wide): N = 4096: B = 48
    // 21.45 / 23.1 ms, 64: 27.34 / 27.4, 80: 33.0 / 33.4, 96: 38.2 / 38.6, 112: 44.6 / 43.9, 128: 49.7 / 48.4; N = 16384,
    // B = 32 (cfg 5): 707.7 / 696.6; 1600 units of N = 3008 (cfg 3): 277.3 / 273.2 -> taken from batch x slabs >= 3400.
    if (n >= 2048 && (long long)batch * ((n + GT - 1) / GT) >= 3400) return 2;
    // The fused panel kernel (128-column panels) is the faster sequence once the batch fills the chip (SF_UNFUSED_BELOW).
    return batch < SF_UNFUSED_BELOW ? 1 : 0;
}
// Every sequence but the unfused one works in a frame shifted by 64 virtual leading rows when n is 64 mod 128
int sf_potrf_front_pad(int n, int batch) {
    if (sf_potrf_pick(n, batch) == 1 || n % GT != 64 || n < 2 * GT) return 0;
    return 64;
}

int sf_launch_potrf(double* A, int n, int lda, int64_t stride, int batch, int* info, double* work,
                    double* rhs, int ldr, hipStream_t s, const sf_gen_args* gen, sf_exec* ex) {
    if (n <= 0 || n % SF_LEAF != 0 || lda < n || batch <= 0 || (lda & 1) || !work) {
        sf_set_error("potrf: n must be a positive multiple of %d, lda >= n and even, workspace required", SF_LEAF);
        return SF_EINVAL;
    }
    // every matrix base must be 16-byte aligned like the first (the panel kernels fetch operands as 16-byte granules:
    // global_load_lds_dwordx4 in the K loops, double2 loads of the L slab and of the partial sums), and the matrices are
    // factorised in place concurrently, so no two may share an element
    if ((stride & 1) || stride < (int64_t)(n - 1) * lda + n) {
        sf_set_error("potrf: stride=%lld must be even and at least (n - 1) lda + n = %lld", (long long)stride,
                     (long long)((int64_t)(n - 1) * lda + n));
        return SF_EINVAL;
    }
    const sf_potrf_scratch ws = sf_potrf_scratch_of(work, n, batch);
    const int seq = sf_potrf_pick(n, batch);
    if (!ex) ex = sf_exec_thread_local();
    // frame of the fused sequences: the caller's (whose tile map was built in it) or this call's own
    const int fp = gen ? gen->fp : sf_potrf_front_pad(n, batch);
    if (seq == 1 && fp == 0) return sf_launch_potrf_v1(A, n, lda, stride, info, ws, rhs, ldr, s, gen, ex);
    // the other sequences work in that frame
    SF_CHECK(sf_check_front_pad(fp, n));
    A -= (int64_t)fp * (lda + 1);
    if (rhs) rhs -= fp;
    n += fp;
    if (seq == 4) return sf_launch_potrf_v4(A, n, lda, stride, info, ws, rhs, ldr, s, gen, fp);
    if (seq == 2 || seq == 3) return sf_launch_potrf_v3(A, n, lda, stride, info, ws, rhs, ldr, s, gen, ex, seq == 3, fp);
    return sf_launch_potrf_v2(A, n, lda, stride, info, ws, rhs, ldr, s, gen, ex, fp);
}
