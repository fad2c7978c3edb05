"""Stand-alone timing of sf_emulator_loglike_grad_batch (the emulator training likelihood and its gradient in the
hyper-parameters) on synthetic libraries.
    python tools/bench_emulator_gradient.py [reps] [train]
Per m M in {216 (m = 8, M = 27), 1320 (m = 4, M = 330: the worked example)} and B in {1, 8, 32}: ms per call of the whole
sf_emulator_loglike_grad_batch, of its contraction launches alone (k_emu_grad of sf_emu_grad.h and k_grad_sum of sf_grad_frame.h, through
sf_debug_emulator_grad_contract on the workspace the call left) and, beside them from the same run, of
sf_emulator_loglike_batch (one likelihood evaluation per row); the call's cost in likelihood evaluations is the ratio.
Second leg (skipped with train = 0): Emulator.train from the defaults three ways -- the serial Nelder-Mead loop,
batch_simplex=True and gradient=True -- with nfev, wall time and the final lnL of each.  At m M = 1320 (17
hyper-parameters) a converged simplex run takes thousands of iterations: there the two simplex runs stop after NM_MAXITER
iterations and the line says so."""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
from _bench_common import timed

from starfish_amd import _device as D
from starfish_amd import _lib, synth
from starfish_amd.emulator import Emulator

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
with_train = int(sys.argv[2]) if len(sys.argv) > 2 else 1
NM_MAXITER = 400  # simplex iterations at m M = 1320 (17 hyper-parameters: a converged run takes thousands)
SIZES = ((8, None), (4, synth.BIG_GRID_AXES))
lib = _lib.require_gpu()
dev = D.device_of()


def emulator(m, axes):
    o = synth.make_order(N=256, m=m, seed=13, grid_axes=axes)
    return Emulator(o["grid_points"], o["param_names"], o["emu_wl"], o["weights"], o["eigenspectra"], o["w_hat"],
                    o["flux_mean"], o["flux_std"], o["factors"])


for m, axes in SIZES:
    emu = emulator(m, axes)
    M, P = emu.grid_points.shape
    S = 1 + m + m * P
    grid, iphiphi, w_hat = (D.to_dev(a, dev) for a in (emu.grid_points, emu.iPhiPhi, emu.w_hat))
    rng = np.random.default_rng(5)
    for B in (1, 8, 32):
        rows = emu._hyper_rows(emu.get_param_vector() + rng.uniform(-0.1, 0.1, (B, S)))
        hyper = D.to_dev(rows, dev)
        lnl, lnl2, grad, grad2 = D.empty((B,), dev), D.empty((B,), dev), D.empty((B, S), dev), D.empty((B, S), dev)
        info = D.empty((B,), dev, torch.int32)
        ws = D.workspace(lib.sf_emulator_loglike_grad_workspace_bytes(M, P, m, B), dev)
        s = D.stream_ptr(dev)
        head = (D.ptr(grid), M, P, m, D.ptr(hyper), S, B, D.ptr(iphiphi))

        def loglike():
            _lib.check(lib.sf_emulator_loglike_batch(*head, D.ptr(w_hat), D.ptr(lnl2), None, None, D.ptr(info), D.ptr(ws),
                                                     ws.numel(), s), "sf_emulator_loglike_batch")

        def whole():
            _lib.check(lib.sf_emulator_loglike_grad_batch(*head, D.ptr(w_hat), D.ptr(lnl), D.ptr(grad), S, D.ptr(info), D.ptr(ws),
                                                          ws.numel(), s), "sf_emulator_loglike_grad_batch")

        def contract():
            _lib.check(lib.sf_debug_emulator_grad_contract(*head, D.ptr(grad2), S, D.ptr(info), D.ptr(ws), ws.numel(), s),
                       "sf_debug_emulator_grad_contract")

        t_ll = timed(loglike, reps)
        t_whole = timed(whole, reps)
        assert int(info.abs().max()) == 0 and bool(torch.isfinite(grad).all()) and torch.equal(lnl, lnl2)
        t_contract = timed(contract, reps)
        assert torch.equal(grad, grad2)
        print(f"m M = {m * M} B = {B}: sf_emulator_loglike_grad_batch {t_whole:8.3f} ms per call, contraction alone "
              f"{t_contract:8.3f} ms, sf_emulator_loglike_batch {t_ll:8.3f} ms: {t_whole / t_ll:.2f} likelihood evaluations",
              flush=True)
        del ws

    if not with_train:
        continue
    n = m * M
    nm_opts = dict(options=dict(maxiter=NM_MAXITER)) if n > 1000 else {}
    for name, kw in (("serial Nelder-Mead", dict(nm_opts)), ("batch_simplex=True", dict(nm_opts, batch_simplex=True)),
                     ("gradient=True", dict(gradient=True))):
        e = emulator(m, axes)
        e.log_likelihood()  # warm-up of each path
        e.log_likelihood_batch(np.tile(e.get_param_vector(), (S + 1, 1)))
        e.log_likelihood_gradient()
        t0 = time.perf_counter()
        try:
            soln = e.train(**kw)
        except np.linalg.LinAlgError as err:  # (a point of the search whose v11 is not positive definite: the run ends there)
            print(f"m M = {n} train from the defaults, {name}: {err} after {(time.perf_counter() - t0) * 1e3:.1f} ms", flush=True)
            continue
        wall = time.perf_counter() - t0
        stopped = "" if soln.success else f" (stopped: {soln.message})"
        print(f"m M = {n} train from the defaults, {name}: nfev {soln.nfev}, nit {soln.nit}, {wall * 1e3:.1f} ms, "
              f"final lnL {-soln.fun!r}{stopped}", flush=True)
