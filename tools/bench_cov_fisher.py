"""Stand-alone timing of sf_fisher_cov_batch (Fisher information of the covariance hyper-parameters) on synthetic orders.
    python tools/bench_cov_fisher.py [reps] [N ...]
Per N in {3008, 4096}, batch 1 and 128, a global kernel and 0 or 4 local kernels (s = 2 or 14 slots), from ONE run: ms per call of
the whole sf_fisher_cov_batch, of its launches behind the inverse alone (k_fc_winv, then k_fc_left, k_fc_contract and k_fc_sum
per slot, through sf_debug_fisher_cov_contract on the workspace the call left), of sf_loglike_grad_batch, and of the 2 s calls of
sf_loglike_grad_batch that a central-difference Hessian of the gradient costs (timed as 2 s calls back to back)."""
import sys

import torch
from _bench_common import order_and_walkers, timed
from gpu_helpers import pack_rows

from starfish_amd import _device as D
from starfish_amd import _lib

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 2
sizes = [int(a) for a in sys.argv[2:]] or [3008, 4096]
lib = _lib.require_gpu()


def with_local_kernels(o, p, n_local):
    """The walker's parameters with n_local local kernels spread over the order, 0.3 pixel off a pixel each (as
    tools/bench_gradient.py places them)."""
    w = o["wave"]
    (_, la, ls), = p["local_cov"]
    at = [(k + 1) * len(w) // (n_local + 1) for k in range(n_local)]
    return dict(p, local_cov=[(float(w[i] + 0.3 * (w[i + 1] - w[i])), la - 0.1 * k, ls + 0.05 * k) for k, i in enumerate(at)])


for N in sizes:
    for B in (1, 128):
        o, do, walkers = order_and_walkers(N, B)
        for n_local in (0, 4):
            md, rows = pack_rows(do, [with_local_kernels(o, p, n_local) for p in walkers])
            dev = do.dev
            s = 2 + 3 * n_local
            with torch.cuda.device(dev):
                P = D.to_dev(rows, dev)
                lnl, lnl2 = D.empty((B,), dev), D.empty((B,), dev)
                F, F2, grad = D.empty((B, s, s), dev), D.empty((B, s, s), dev), D.empty((B, s), dev)
                info = D.empty((B,), dev, torch.int32)
                ws = do._reserve(max(do.fisher_cov_workspace_bytes(md, B), do.loglike_grad_workspace_bytes(md, B)))

                def gradient():
                    do._call("loglike_grad_batch", md, B, P, lnl2, grad, s, None, info, ws=ws)

                def difference_hessian():
                    for _ in range(2 * s):
                        gradient()

                one = timed(gradient, reps)
                fd = timed(difference_hessian, reps)
                whole = timed(lambda: do._call("fisher_cov_batch", md, B, P, lnl, F, s * s, info, ws=ws), reps)
                assert int(info.abs().max()) == 0 and bool(torch.isfinite(F).all()) and torch.equal(lnl, lnl2)
                behind = timed(lambda: do._call("debug_fisher_cov_contract", md, B, P, F2, s * s, ws=ws), reps)
                assert torch.equal(F, F2) and torch.equal(F, F.transpose(1, 2))
                do.release_workspace()
                del ws
            print(f"N={N} B={B} global + {n_local} local kernels (s = {s}): sf_fisher_cov_batch {whole:9.3f} ms per call, behind the "
                  f"inverse alone {behind:9.3f} ms, sf_loglike_grad_batch {one:8.3f} ms, {2 * s} x sf_loglike_grad_batch {fd:9.3f} ms "
                  f"= {fd / whole:.1f} x the Fisher call ({reps} calls each)", flush=True)
