"""Stand-alone timing of sf_loglike_banded_mean_grad_batch (the mean-flux gradient on the band + Woodbury solver).
    python tools/bench_banded_gradient.py N B [reps] [runs]
On the synthetic order of N pixels (m = 4, a global and one local kernel) with B walkers around its truth and the eight mean
labels of synth.LABELS, in ONE process: ms per call of the new call, of sf_loglike_banded_batch (the banded likelihood alone)
and of the dense sf_loglike_mean_grad_batch, all at the walkers' largest host half-width bound.  The three are timed in turn,
``reps`` calls each (default 10; one more in front is not timed), and the turn is repeated ``runs`` times (default 5): printed
are the median over the runs and their range.  Before the timing the banded gradient is compared with the dense one."""
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
assert W <= do.banded_window_halfwidth(), (W, do.banded_window_halfwidth())
with torch.cuda.device(dev):
    P = D.to_dev(rows, dev)
    lnl, lnl_b, lnl_d = D.empty((B,), dev), D.empty((B,), dev), D.empty((B,), dev)
    grad, grad_d = D.empty((B, P8), dev), D.empty((B, P8), dev)
    info = D.empty((B,), dev, torch.int32)
    ws = do._reserve(max(do.loglike_banded_mean_grad_workspace_bytes(md, B, W, P8), do.loglike_mean_grad_workspace_bytes(md, B, P8),
                         do.banded_workspace_bytes(md, B, W)))
    calls = {
        "sf_loglike_banded_mean_grad_batch": lambda: do._call("loglike_banded_mean_grad_batch", md, B, P, W, h_slots, P8, lnl, grad, P8,
                                                              None, info, ws=ws),
        "sf_loglike_banded_batch": lambda: do._call("loglike_banded_batch", md, B, P, W, lnl_b, None, None, None, None, info, ws=ws),
        "sf_loglike_mean_grad_batch (dense)": lambda: do._call("loglike_mean_grad_batch", md, B, P, h_slots, P8, lnl_d, grad_d, P8,
                                                               None, info, ws=ws),
    }
    for call in calls.values():
        call()
        torch.cuda.synchronize()
        assert int(info.abs().max()) == 0
    scale = grad_d.abs().amax(dim=0)
    print(f"N={N} B={B} half-width {W}: max |banded - dense| per column / max |dense|: "
          f"{((grad - grad_d).abs().amax(dim=0) / scale).max().item():.3g}; max |lnl - dense lnl| / |lnl| "
          f"{((lnl - lnl_d).abs() / lnl_d.abs()).max().item():.3g}", flush=True)
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
new, like, dense = (med[name] for name in calls)
print(f"N={N} B={B}: banded gradient = {new / like:.2f} banded likelihoods, dense gradient = {dense / new:.2f} banded gradients",
      flush=True)
