// Per-spectrum transform kernels for gfx950 (all fp64; compiled with -ffp-contract=off so element
// formulas keep the reference's operation order):
//   k_broaden        rfft -> kernel multiply -> irfft     Starfish/transforms.py:45-90, 93-134
//   k_spline_solve   banded (LU) solve of the k=5 B-spline collocation system  (transforms.py:39-42,
//                    FITPACK curfit with s=0; knots x[0]x6, x[3:-3], x[-1]x6)
//   k_eval_rows      doppler_shift + spline evaluation + chebyshev_correct + eigenspectrum
//                    reconstruction      transforms.py:137-158, 271-304; spectrum_model.py:293-313
//   k_scale, k_resid_y   rescale / renorm, residual and the rank-m factor Y   spectrum_model.py:316-335
//   k_emu_prep/z/post GP conditional of the PCA weights     Starfish/emulator/emulator.py:330-394
//   k_v11_build(_batch)   the covariance of the emulator-training likelihood      emulator.py:126-128,569-571
//
// ONE translation unit; layers are headers, every launcher directly below its kernel:
//   sf_transform_fft.h      FFT bodies, multipliers, k_broaden, k_kernel_mult, k_broaden_half, k_rfft_rows
//   sf_transform_spline.h   k_spline_solve, k_spline_apply, the B-spline basis / interval search, k_spline_eval
//   sf_transform_eval.h     Chebyshev, extinction laws, sf_eval_pixel, k_eval_rows, k_scale, k_resid_y, k_eval_resid_y
//   sf_transform_emu.h      k_emu_prep/z/post, k_emu_joint, k_finish
//   sf_transform_v11.h      k_v11_build, k_v11_build_batch
//   sf_mean_grad.h          the gradient in the mean-flux parameters: k_mean_stage, k_mean_finish, k_mean_pixel, k_mean_sum
//   sf_fisher.h             the Fisher information of the mean-flux parameters: k_fisher_tangent, k_fisher_band, k_fisher_ztz
//   sf_fisher_multi.h       the Fisher matrices of a multi-order call: k_fisher_spread, k_multi_fisher_reduce
//   sf_local_scan_multi.h   the averaged proposal of a score scan: k_ls_mean
#include "sf_common.h"
#include "sf_device.h"
#include "sf_transform.h"
#include "sf_transform_fft.h"
#include "sf_transform_spline.h"
#include "sf_transform_eval.h"
#include "sf_transform_emu.h"
#include "sf_transform_v11.h"
#include "sf_mean_grad.h"
#include "sf_fisher.h"
#include "sf_fisher_multi.h"
#include "sf_local_scan_multi.h"
