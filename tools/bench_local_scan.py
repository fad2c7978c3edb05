"""Stand-alone timing of sf_local_scan_batch (score scan for new local kernels) on synthetic orders.
    python tools/bench_local_scan.py [reps] [N ...]
Per N in {3008, 4096}, batch 1 and 128, the walkers' own model (a global and one local kernel), every pixel x the widths 8, 15 and
30 km/s as candidates (3 N of them), from ONE run: ms per call of the whole sf_local_scan_batch, of its launches behind the inverse
alone (k_ls_wband, k_ls_patch, k_ls_cand through sf_debug_local_scan_contract on the workspace the call left), of
sf_pointwise_batch (the same head: factor, solve, inverse factor) and of one sf_loglike_grad_batch (what a scan by tiny added
kernels costs per candidate and batch, and it gives the score only)."""
import sys

import numpy as np
import torch
from _bench_common import order_and_walkers, timed
from gpu_helpers import pack_rows

from starfish_amd import _device as D
from starfish_amd import _lib

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 2
sizes = [int(a) for a in sys.argv[2:]] or [3008, 4096]
lib = _lib.require_gpu()
SIGMAS = (8.0, 15.0, 30.0)

for N in sizes:
    for B in (1, 128):
        o, do, walkers = order_and_walkers(N, B)
        md, rows = pack_rows(do, walkers)
        dev = do.dev
        cand = np.array([(w, s) for s in SIGMAS for w in o["wave"]])
        ncand = len(cand)
        with torch.cuda.device(dev):
            P, Cd = D.to_dev(rows, dev), D.to_dev(cand, dev)
            lnl, lnl2 = D.empty((B,), dev), D.empty((B,), dev)
            out, out2 = D.empty((B, ncand, 3), dev), D.empty((B, ncand, 3), dev)
            alpha, cinv_diag, grad = D.empty((B, 1, N), dev), D.empty((B, N), dev), D.empty((B, 5), dev)
            info = D.empty((B,), dev, torch.int32)
            ws = do._reserve(max(do.local_scan_workspace_bytes(md, B, ncand), do.pointwise_workspace_bytes(md, B, 1),
                                 do.loglike_grad_workspace_bytes(md, B)))
            head = timed(lambda: do._call("pointwise_batch", md, B, P, None, 1, N, 0, alpha, cinv_diag, None, None, info, ws=ws), reps)
            one = timed(lambda: do._call("loglike_grad_batch", md, B, P, lnl2, grad, 5, None, info, ws=ws), reps)
            whole = timed(lambda: do._call("local_scan_batch", md, B, P, Cd, ncand, out, lnl, info, ws=ws), reps)
            assert int(info.abs().max()) == 0 and bool(torch.isfinite(out).all()) and torch.equal(lnl, lnl2)
            behind = timed(lambda: do._call("debug_local_scan_contract", md, B, P, Cd, ncand, out2, ws=ws), reps)
            assert torch.equal(out, out2)
            do.release_workspace()
            del ws
        print(f"N={N} B={B} {ncand} candidates: sf_local_scan_batch {whole:9.3f} ms per call, behind the inverse alone {behind:9.3f} ms, "
              f"sf_pointwise_batch {head:8.3f} ms, sf_loglike_grad_batch {one:8.3f} ms; one gradient call per candidate would be "
              f"{ncand * one / whole:.0f} x the scan ({reps} calls each)", flush=True)
