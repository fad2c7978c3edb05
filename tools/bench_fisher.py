"""Stand-alone timing of the Fisher information of the mean-flux parameters (sf_fisher_banded_mean_batch, sf_fisher_mean_batch).
    python tools/bench_fisher.py N B [reps] [runs]
On the synthetic order of N pixels (m = 4, a global and one local kernel) with B walkers around its truth and the eight mean
labels of synth.LABELS, in ONE process: ms per call of the banded Fisher call, of sf_loglike_banded_batch (the banded
likelihood alone), of sf_loglike_banded_mean_grad_batch, of the dense Fisher call, of sf_loglike_batch and of 2 p banded
gradient calls (what central differences of the gradient would cost), the banded ones at the walkers' largest host half-width
bound.  The calls are timed in turn, ``reps`` calls each (default 10; one more in front is not timed), and the turn is repeated
``runs`` times (default 5): printed are the median over the runs and their range.  Before the timing the banded matrix is
compared with the dense one."""
import ctypes as C
import statistics
import sys

N, B = int(sys.argv[1]), int(sys.argv[2])
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
runs = int(sys.argv[4]) if len(sys.argv) > 4 else 5

import torch  # noqa: E402
from _bench_common import order_and_walkers, timed  # noqa: E402
from gpu_helpers import pack_rows  # noqa: E402

from starfish_amd import _device as D  # noqa: E402
from starfish_amd import _lib  # noqa: E402

lib = _lib.require_gpu()
o, do, walkers = order_and_walkers(N, B)
md, rows = pack_rows(do, walkers)
dev = do.dev
cols = [1, 0, 2, 6 + do.P, 7 + do.P, 6, 7, 8]
P8 = len(cols)
h_slots = (C.c_int * P8)(*cols)
W = int(do.halfwidth_bound(md, rows).max())
assert do.fisher_banded_max_slots(W) >= P8, (W, do.fisher_banded_max_slots(W))
with torch.cuda.device(dev):
    P = D.to_dev(rows, dev)
    lnl, lnl_b, lnl_d, lnl_g = (D.empty((B,), dev) for _ in range(4))
    F, F_d = D.empty((B, P8, P8), dev), D.empty((B, P8, P8), dev)
    grad = D.empty((B, P8), dev)
    info = D.empty((B,), dev, torch.int32)
    ws = do._reserve(max(do.fisher_banded_mean_workspace_bytes(md, B, W, P8), do.fisher_mean_workspace_bytes(md, B, P8),
                         do.loglike_banded_mean_grad_workspace_bytes(md, B, W, P8), do.banded_workspace_bytes(md, B, W),
                         do.workspace_bytes(md, B)))

    def banded_gradient():
        do._call("loglike_banded_mean_grad_batch", md, B, P, W, h_slots, P8, lnl_g, grad, P8, None, info, ws=ws)

    def finite_differences():
        for _ in range(2 * P8):
            banded_gradient()

    calls = {
        "sf_fisher_banded_mean_batch": lambda: do._call("fisher_banded_mean_batch", md, B, P, W, h_slots, P8, lnl, F, P8 * P8, None, info,
                                                        ws=ws),
        "sf_loglike_banded_batch": lambda: do._call("loglike_banded_batch", md, B, P, W, lnl_b, None, None, None, None, info, ws=ws),
        "sf_loglike_banded_mean_grad_batch": banded_gradient,
        "sf_fisher_mean_batch (dense)": lambda: do._call("fisher_mean_batch", md, B, P, h_slots, P8, lnl_d, F_d, P8 * P8, info, ws=ws),
        "sf_loglike_batch (dense)": lambda: do._call("loglike_batch", md, B, P, lnl_b, None, None, None, None, info, ws=ws),
        f"{2 * P8} x sf_loglike_banded_mean_grad_batch": finite_differences,
    }
    for call in calls.values():
        call()
        torch.cuda.synchronize()
        assert int(info.abs().max()) == 0
    d = F_d.diagonal(dim1=1, dim2=2).sqrt()
    scale = d[:, :, None] * d[:, None, :]
    print(f"N={N} B={B} half-width {W}: max |banded - dense| / sqrt(F_ii F_jj) {((F - F_d).abs() / scale).max().item():.3g}; "
          f"max |lnl - dense lnl| / |lnl| {((lnl - lnl_d).abs() / lnl_d.abs()).max().item():.3g}", flush=True)
    times = {name: [] for name in calls}
    for _ in range(runs):
        for name, call in calls.items():
            times[name].append(timed(call, reps))
    do.release_workspace()
    del ws
med = {name: statistics.median(v) for name, v in times.items()}
for name, v in times.items():
    print(f"N={N} B={B} {name}: {med[name]:8.3f} ms per call (median of {runs} runs of {reps} calls; {min(v):.3f} .. {max(v):.3f})",
          flush=True)
new, like, gradient, dense, dense_like, fd = (med[name] for name in calls)
print(f"N={N} B={B}: banded Fisher = {new / like:.2f} banded likelihoods = {new / gradient:.2f} banded gradients; dense Fisher = "
      f"{dense / dense_like:.2f} dense likelihoods = {dense / new:.2f} banded Fisher; {2 * P8} banded gradients = {fd / new:.1f} "
      "banded Fisher", flush=True)
