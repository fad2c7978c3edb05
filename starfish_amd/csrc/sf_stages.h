// Stages of the likelihood that the single-order, multi-order, banded and factor-applied sequences share (internal;
// sf_abi.cpp).
#pragma once
#include "sf_prof.h"
#include "sf_work.h"

#pragma GCC visibility push(hidden)
// Prologue of every single-order entry point: arguments and workspace size checked, the context's device selected,
// the workspace carved
int open_call(const sf_ctx* c, const sf_model_desc* mdl, int B, void* d_work, size_t have, bool need_C, Work* w);
// emulator + transform chain -> unscaled X / flux, scale, then residual / Y
int run_transforms(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params, const Work& w, double* d_flux_out,
                   double* d_X_out, double* d_resid_out, double* d_log_scale, bool want_Y, hipStream_t s);
// the arguments of the emulator's, the broadening's and the per-pixel evaluation's launches on the workspace w, as
// run_transforms hands them to its kernels
sf_emu_args emu_args(sf_ctx* c, const sf_model_desc* mdl, const double* d_params, const Work& w, double* d_mu, double* d_cov,
                     double* d_Lw, int* d_info);
sf_broaden_args broaden_args(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params, const Work& w);
sf_eval_args eval_args(sf_ctx* c, const sf_model_desc* mdl, const double* d_params, const Work& w);
sf_fill_args fill_args(sf_ctx* c, const sf_model_desc* mdl, const double* d_params, const Work& w);
// The likelihood's fill of the workspace matrices of layout L (lower tiles, identity padding, jitter), in the frame fp of
// the factorisation: only the tiles that carry more than the rank-m term are materialised (tile map and list)
sf_fill_args loglike_fill_args(sf_ctx* c, const sf_model_desc* mdl, const double* d_params, const Work& w, const Layout& L, int fp);
// The rest of the likelihood of `units` matrices filled that way: the factorisation, whose generator (Y, tile map, same
// frame) supplies the tiles the fill left out and through which the residual rides (w.resid becomes z = L^-1 R); then
// logdet and the squared Mahalanobis distance -> lnL.  ltbuf: the factorisation's scratch, ex: its executor.
int loglike_factor_finish(const Work& w, const Layout& L, int fp, int units, double* ltbuf, double* d_lnl, int* d_info,
                          hipStream_t s, sf_exec* ex);
// optional results of `units` units, copied out of the workspace behind everything enqueued on s
int export_info(int* d_info, const Work& w, int units, hipStream_t s);
int export_logdet_sqmah(double* d_logdet, double* d_sqmah, const Work& w, int units, hipStream_t s);
// The mean gradient's own checks of one request (behind model_ok): a model it differentiates, 1 .. SF_MEAN_GRAD_MAX_SLOTS columns
// that are mean-flux parameters of it, none twice, and rows that hold them.  who: how the message starts
bool mean_counts_ok(const sf_model_desc* mdl, int nslots);  // its model and slot-count conditions alone, silently (size queries)
int mean_slots_ok(const char* who, const sf_ctx* c, const sf_model_desc* mdl, const int* h_slots, int nslots, int grad_stride);
// What sf_fisher_mean_batch and sf_fisher_banded_mean_batch refuse before they look at the context: a required pointer that is
// NULL (required == false), nslots outside 1 .. SF_MEAN_GRAD_MAX_SLOTS, fisher_stride < nslots^2
int fisher_counts_ok(const char* who, bool required, int nslots, int fisher_stride);
// the arguments of the mean gradient's launches: the staging area, moments, partial sums and tangents of aw on the workspace w
// (rows of w.L.npad doubles), nslots columns into d_grad
sf_mean_grad_args mean_grad_kernel_args(const sf_ctx* c, const int* h_slots, int nslots, const Work& w, const AppliedWork& aw,
                                        double* d_grad, int grad_stride);
#pragma GCC visibility pop
