// Structure-exploiting solver for the likelihood:
//
//     C  =  Bd  +  Y^T Y ,      Bd = diag(sigma^2) + K_global + sum K_local + 1e-10 I
//
// The reference builds C dense (Starfish/models/spectrum_model.py:334-363) although K_global and
// K_local are compactly supported (the `r <= r0` masks of Starfish/models/kernels.py:33,78), so Bd is
// a band matrix of half-width W pixels (24 ls/dv for the global kernel, whose metric is a quarter of
// the velocity separation) and Y^T Y = X^T Sigma_w^-1 X has rank m.  With
//     Bd = L L^T (banded),  z = L^-1 R,  Z = L^-1 Y^T,   S = I_m + Z^T Z = L_S L_S^T
//     logdet C = logdet Bd + logdet S
//     R^T C^-1 R = z^T z - | L_S^-1 Z^T z |^2                        (Woodbury)
// only forward substitutions are needed and the cost drops from N^3/3 to O(N W^2) flops per walker.
//
// k_band_forms: one workgroup per matrix sweeps the band in 16-column steps over a sliding window of
// (W+16) rows held in LDS.  The window is stored as 16 x 16 blocks addressed by the UNORDERED pair of
// ring slots {row block % nbr, column block % nbr}: every live block of the lower triangle has its own
// slot, nothing is ever shifted, and the footprint is nbr(nbr+1)/2 blocks instead of nbr^2.
// Everything runs on v_mfma_f64_16x16x4_f64.  Per step k (columns 16k .. 16k+15):
//   wave 0   runs the sequential chain by itself, free of barriers: it factorises the diagonal block k AND
//            inverts its factor in the MFMA accumulator layout (one rank-1 MFMA per column each, pivots from
//            scalars so that the rsqrt chain overlaps the matrix core), publishes F_k = L_kk^-1, solves the
//            next sub-diagonal block X_{k+1,k} = A_{k+1,k} F_k^T, applies it to the next diagonal block and
//            goes on with k+1;
//   waves 1+ ("workers") trail by one column: they solve the rest of block column k as products with F_k,
//            apply column k to the window (software pipelined: operands of the next block are read under
//            the MFMAs of the current one), fetch the next 16 band rows / right-hand-side columns from HBM
//            into registers and drop them into the slots column k retires.
// LDS flags order the two sides; the workers meet at two LDS-counter barriers per column.  Block addresses
// depend on the ring phase k % nbr only: each wave tabulates its operations once (lane = phase) and reads
// them back with one v_readlane per operation.
// The right-hand sides (residual + the m rows of Y) ride along as extra ROWS of the matrix, so their
// forward substitution is the same solve/update, and their Gram matrix [z Z]^T [z Z] accumulates in
// LDS.  L is never written anywhere: the outputs are logdet(Bd) and the (1+m)^2 Gram matrix.
// k_woodbury then does the m x m capacitance solve.
// Measured on MI355X (cfg 2, W = 141 px, 16 waves): 1.27 ms for 128 matrices = one CU each (11.5k cycles
// per column against 4.7k of MFMA time: 296 MFMAs x 64 cycles over four SIMDs).  While 2*batch workgroups
// fit the chip the sweep is therefore "twisted": one workgroup eliminates the first half of the columns
// top-down, a second one the last half bottom-up (same code on the index-reversed matrix), both dump what
// is left of a (W rounded up to 16)-row separator, k_band_merge adds the two Schur contributions and a
// short third sweep finishes the separator: 0.74 ms.
//
// ONE translation unit; layers are headers, every launcher directly below its kernel:
//   sf_band_shape.h     the window's shape without HIP: constants, nbr / nrb / waves, the LDS layout, which solver takes a
//                       half-width, the workers' positions, the twisted sweep's shape and workspace, when it pays
//   sf_band_window.h    sf_band_args, sfb_pair, sfb_gram, sfb_fetch (the right-hand sides and the call: sf_band_rhs, sf_band_call, sf_common.h)
//   sf_band_sweep.h     k_band_forms (its text: sf_band_sweep_body.h), launch_forms_kernel, sf_launch_band_forms
//   sf_band_twist.h     k_band_merge, sf_band_twisted_applicable, sf_launch_band_forms_twisted
//   sf_band_woodbury.h  k_woodbury, sf_launch_woodbury
//   sf_band_solve.h     the full solve x = A^-1 rhs for the mean-flux gradient: k_band_keep (the sweep, which then also stores
//                       the factor), k_band_back (backward sweep), k_band_mix_matrix / k_band_mix (Woodbury mix), their launchers
//   sf_band_selinv.h    for the covariance gradient on the band: k_band_selinv (selected inversion: the band of Bd^-1 from the
//                       kept factor), k_band_vs_matrix (Vs of C^-1 = Bd^-1 - Vs Vs^T through k_band_mix), their launchers (the
//                       contraction with dC / d theta over the band is sf_fill.hip's, beside the derivative formulas)
//   sf_band_diag.h      for the residual diagnostics on the band: k_band_diag_stage (the sweep's rows [R; Y] for caller
//                       right-hand sides), k_band_cinv_diag (diag(C^-1) = diag(Sigma) - rowsum(Vs^2)), k_band_cov_diag, their
//                       launchers (the split by covariance component is sf_fill.hip's sf_launch_cov_matvec)
#include "sf_common.h"
#include "sf_device.h"
#include "sf_band_shape.h"
#include "sf_band_window.h"
#include "sf_band_sweep.h"
#include "sf_band_twist.h"
#include "sf_band_woodbury.h"
#include "sf_band_solve.h"
#include "sf_band_selinv.h"
#include "sf_band_diag.h"
