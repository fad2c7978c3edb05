"""Stand-alone timing of sf_loglike_grad_batch (likelihood gradient in the covariance hyper-parameters) on synthetic orders.
    python tools/bench_gradient.py [reps] [B] [N ...]
Per N in {3008, 4096}, batch 128, a global kernel and 0 or 4 local kernels: ms per call of the whole sf_loglike_grad_batch, of
its contraction launches alone (k_cov_grad of sf_cov_grad.h and k_grad_sum of sf_grad_frame.h, through sf_debug_loglike_grad_contract on the
workspace the call left) and, beside them from the same run, of sf_pointwise_batch (the same sequence up to and including the
inverse's launches) and of sf_loglike_batch (one likelihood evaluation)."""
import torch
from _bench_common import arguments, order_and_walkers, timed
from gpu_helpers import pack_rows

from starfish_amd import _device as D
from starfish_amd import _lib

reps, B, sizes = arguments(3)
lib = _lib.require_gpu()


def with_local_kernels(o, p, n_local):
    """The walker's parameters with n_local local kernels spread over the order, 0.3 pixel off a pixel each."""
    w = o["wave"]
    (_, la, ls), = p["local_cov"]
    at = [(k + 1) * len(w) // (n_local + 1) for k in range(n_local)]
    return dict(p, local_cov=[(float(w[i] + 0.3 * (w[i + 1] - w[i])), la - 0.1 * k, ls + 0.05 * k) for k, i in enumerate(at)])


for N in sizes:
    o, do, walkers = order_and_walkers(N, B)
    for n_local in (0, 4):
        md, rows = pack_rows(do, [with_local_kernels(o, p, n_local) for p in walkers])
        dev, n = do.dev, do.n
        slots = 2 + 3 * n_local
        with torch.cuda.device(dev):
            P = D.to_dev(rows, dev)
            lnl, lnl2, grad, grad2 = D.empty((B,), dev), D.empty((B,), dev), D.empty((B, slots), dev), D.empty((B, slots), dev)
            alpha, cinv_diag = D.empty((B, 1, n), dev), D.empty((B, n), dev)
            info = D.empty((B,), dev, torch.int32)
            ws = do._reserve(max(do.loglike_grad_workspace_bytes(md, B), do.pointwise_workspace_bytes(md, B, 1)))
            pointwise = timed(lambda: do._call("pointwise_batch", md, B, P, None, 1, n, 0, alpha, cinv_diag, None, None, info, ws=ws),
                              reps)
            loglike = timed(lambda: do._call("loglike_batch", md, B, P, lnl2, None, None, None, None, info, ws=ws), reps)
            whole = timed(lambda: do._call("loglike_grad_batch", md, B, P, lnl, grad, slots, None, info, ws=ws), reps)
            assert int(info.abs().max()) == 0 and bool(torch.isfinite(grad).all()) and torch.equal(lnl, lnl2)
            contract = timed(lambda: do._call("debug_loglike_grad_contract", md, B, P, grad2, slots, ws=ws), reps)
            assert torch.equal(grad, grad2)
            do.release_workspace()
            del ws
        print(f"N={N} B={B} global + {n_local} local kernels: sf_loglike_grad_batch {whole:8.3f} ms per call, contraction alone "
              f"{contract:8.3f} ms, sf_pointwise_batch {pointwise:8.3f} ms, sf_loglike_batch {loglike:8.3f} ms", flush=True)
