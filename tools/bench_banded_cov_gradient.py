"""Stand-alone timing of sf_loglike_banded_grad_batch (the covariance gradient on the band + Woodbury solver).
    python tools/bench_banded_cov_gradient.py N B [reps] [runs]
On the synthetic order of N pixels (m = 4, a global and one local kernel) with B walkers around its truth, in ONE process: ms
per call of the covariance-only call (no mean slots), of the combined call (the eight mean labels of synth.LABELS and the
covariance slots), of sf_loglike_banded_batch (the banded likelihood alone) and of the dense sf_loglike_grad_batch, all at the
walkers' largest host half-width bound.  The four are timed in turn, ``reps`` calls each (default 10; one more in front is not
timed), and the turn is repeated ``runs`` times (default 5): printed are the median over the runs and their range.  Before the
timing the banded covariance columns are compared with the dense ones."""
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
from starfish_amd import _rows as R  # noqa: E402

lib = _lib.require_gpu()
o, do, walkers = order_and_walkers(N, B)
md, rows = pack_rows(do, walkers)
dev = do.dev
cols = [1, 0, 2, 6 + do.P, 7 + do.P, 6, 7, 8]
P8, ncov = len(cols), R.cov_grad_slots(md)
h_slots = (C.c_int * P8)(*cols)
W = int(do.halfwidth_bound(md, rows).max())
assert W <= do.banded_window_halfwidth(), (W, do.banded_window_halfwidth())
with torch.cuda.device(dev):
    P = D.to_dev(rows, dev)
    lnl, lnl_c, lnl_b, lnl_d = (D.empty((B,), dev) for _ in range(4))
    grad, grad_c, grad_d = D.empty((B, ncov), dev), D.empty((B, P8 + ncov), dev), D.empty((B, ncov), dev)
    info = D.empty((B,), dev, torch.int32)
    ws = do._reserve(max(do.loglike_banded_grad_workspace_bytes(md, B, W, P8, True), do.loglike_grad_workspace_bytes(md, B),
                         do.banded_workspace_bytes(md, B, W)))
    calls = {
        "sf_loglike_banded_grad_batch (covariance only)": lambda: do._call("loglike_banded_grad_batch", md, B, P, W, h_slots, 0, 1, lnl,
                                                                           grad, ncov, None, info, ws=ws),
        "sf_loglike_banded_grad_batch (8 mean + covariance)": lambda: do._call("loglike_banded_grad_batch", md, B, P, W, h_slots, P8, 1,
                                                                               lnl_c, grad_c, P8 + ncov, None, info, ws=ws),
        "sf_loglike_banded_batch": lambda: do._call("loglike_banded_batch", md, B, P, W, lnl_b, None, None, None, None, info, ws=ws),
        "sf_loglike_grad_batch (dense)": lambda: do._call("loglike_grad_batch", md, B, P, lnl_d, grad_d, ncov, None, info, ws=ws),
    }
    for call in calls.values():
        call()
        torch.cuda.synchronize()
        assert int(info.abs().max()) == 0
    scale = grad_d.abs().amax(dim=0)
    assert torch.equal(grad_c[:, P8:], grad)
    print(f"N={N} B={B} half-width {W}: max |banded - dense| per covariance column / max |dense|: "
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
cov, both, like, dense = (med[name] for name in calls)
print(f"N={N} B={B}: covariance gradient = {cov / like:.2f} banded likelihoods, combined = {both / like:.2f}; dense gradient = "
      f"{dense / cov:.2f} banded covariance gradients", flush=True)
