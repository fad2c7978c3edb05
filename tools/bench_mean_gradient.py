"""Stand-alone timing of sf_loglike_mean_grad_batch (likelihood gradient in the mean-flux parameters) on synthetic orders.
    python tools/bench_mean_gradient.py [reps] [B] [N ...]
Per N in {3008, 4096}, batch 128, the eight mean labels of synth.LABELS (vz, vsini, log_scale, cheb:1, cheb:2, T, logg, Z): ms
per call of the whole sf_loglike_mean_grad_batch, of the launches behind its solve alone (k_mean_moments, k_mean_finish,
k_mean_pixel, k_mean_grid, k_mean_sum of sf_mean_grad.h, through sf_debug_loglike_mean_grad_contract on the workspace the call
left) and, beside them from the same run, of sf_loglike_batch (one likelihood evaluation) and of the 2 P likelihood evaluations
that central differences in the P = 8 labels take."""
import ctypes as C

import torch
from _bench_common import arguments, order_and_walkers, timed
from gpu_helpers import pack_rows

from starfish_amd import _device as D
from starfish_amd import _lib

reps, B, sizes = arguments(3)
lib = _lib.require_gpu()

for N in sizes:
    o, do, walkers = order_and_walkers(N, B)
    md, rows = pack_rows(do, walkers)
    dev = do.dev
    cols = [1, 0, 2, 6 + do.P, 7 + do.P, 6, 7, 8]
    P8 = len(cols)
    h_slots = (C.c_int * P8)(*cols)
    with torch.cuda.device(dev):
        P = D.to_dev(rows, dev)
        lnl, lnl2, grad, grad2 = D.empty((B,), dev), D.empty((B,), dev), D.empty((B, P8), dev), D.empty((B, P8), dev)
        info = D.empty((B,), dev, torch.int32)
        ws = do._reserve(do.loglike_mean_grad_workspace_bytes(md, B, P8))
        loglike = timed(lambda: do._call("loglike_batch", md, B, P, lnl2, None, None, None, None, info, ws=ws), reps)

        def central_differences():
            for _ in range(2 * P8):
                do._call("loglike_batch", md, B, P, lnl2, None, None, None, None, info, ws=ws)

        differences = timed(central_differences, reps)
        whole = timed(lambda: do._call("loglike_mean_grad_batch", md, B, P, h_slots, P8, lnl, grad, P8, None, info, ws=ws), reps)
        assert int(info.abs().max()) == 0 and bool(torch.isfinite(grad).all()) and torch.equal(lnl, lnl2)
        contract = timed(lambda: do._call("debug_loglike_mean_grad_contract", md, B, P, h_slots, P8, grad2, P8, ws=ws), reps)
        assert torch.equal(grad, grad2)
        do.release_workspace()
        del ws
    print(f"N={N} B={B} {P8} mean labels: sf_loglike_mean_grad_batch {whole:8.3f} ms per call ({whole / loglike:.2f} likelihood "
          f"evaluations), behind the solve alone {contract:8.3f} ms, sf_loglike_batch {loglike:8.3f} ms, {2 * P8} evaluations for "
          f"central differences {differences:8.3f} ms", flush=True)
