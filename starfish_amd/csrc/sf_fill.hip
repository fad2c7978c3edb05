// Fused covariance fill for gfx950: one pass writes
//     C[b] = Y_b^T Y_b  +  diag(sigma^2)  +  K_global  +  sum_k K_local,k  (+ 1e-10 I)
// replacing the dense temporaries of the reference:
//   Starfish/models/spectrum_model.py:334-363  (X^T Sigma_w^-1 X, fill_diagonal, cov += ...)
//   Starfish/models/kernels.py:7-41            (global_covariance_matrix)
//   Starfish/models/kernels.py:44-81           (local_covariance_matrix)
//   Starfish/models/spectrum_model.py:399      (jitter)
// The rank-m emulator term runs on v_mfma_f64_16x16x4_f64 (the MFMA row index is mapped to matrix
// COLUMNS so that every lane owns 4 consecutive columns -> 32-byte stores, full 128-B lines per
// 4 lanes); the banded/patch kernels are evaluated only in wave sub-tiles that intersect their
// support.  Compiled with -ffp-contract=off: element formulas keep the reference's operation order.
//
// ONE translation unit; layers are headers, every launcher directly below its kernels:
//   sf_fill_elem.h    sf_matern_elem, sf_local_elem, the hyper-parameter read-out, sf_block_support, host-side checks
//   sf_fill_band.h    k_band_gtab, k_band_fill: band storage for sf_band.hip (and the likelihood's per-diagonal table)
//   sf_fill_tile.h    sf_rank_m_subtile, sf_tile_finish, k_tile_map, k_fill_tiles, k_fill_tiles_list: the likelihood path
//   sf_fill_dense.h   k_dense_map, k_fill_dense_plain, k_fill_dense_band: both triangles of caller matrices
//   sf_fill_free.h    k_global_cov, k_local_cov, k_stream_write: stand-alone kernels and the write probe
//   sf_cov_matvec.h   k_cov_yv, k_cov_matvec: the components of C applied to vectors (sf_decompose_batch)
//   sf_cinv.h         sf_cinv_tile, k_cinv_blocks: 64 x 64 blocks of C^-1 from the inverse factor
//   sf_grad_frame.h   sf_grad_tile, sf_grad_flush, k_grad_sum, sf_launch_grad: what the two likelihood gradients share; k_multi_grad_reduce
//   sf_cov_grad.h     k_cov_grad: the likelihood's gradient in the covariance hyper-parameters
//   sf_fisher_cov.h   k_fc_winv, k_fc_left, k_fc_contract, k_fc_sum: the Fisher information of those hyper-parameters
//   sf_local_scan.h   k_ls_wband, k_ls_patch, k_ls_cand: the score scan for a new local kernel at amplitude 0
//   sf_band_local_scan.h  k_ls_wband_banded: the band of C^-1 for that scan from the band solver's selected inversion and Vs
//   sf_band_cov_grad.h  k_band_cov_grad: the same gradient contracted over the band of Bd^-1 and the low-rank correction
//   sf_emu_grad.h     k_emu_grad: the emulator training likelihood's gradient in its hyper-parameters
#include "sf_common.h"
#include "sf_device.h"
#include "sf_fill_elem.h"
#include "sf_fill_band.h"
#include "sf_fill_tile.h"
#include "sf_fill_dense.h"
#include "sf_fill_free.h"
#include "sf_cov_matvec.h"
#include "sf_cinv.h"
#include "sf_grad_frame.h"
#include "sf_cov_grad.h"
#include "sf_fisher_cov.h"
#include "sf_local_scan.h"
#include "sf_band_local_scan.h"
#include "sf_band_cov_grad.h"
#include "sf_emu_grad.h"
