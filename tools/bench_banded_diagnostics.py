"""Stand-alone timing of the residual diagnostics on the band + Woodbury solver against the dense factor.
    python tools/bench_banded_diagnostics.py [N] [reps] [runs]
On the synthetic order of N pixels (default 4096; m = 4, a global and one local kernel), in ONE process: wall-clock ms per call of
SpectrumModel.pointwise_batch and residual_components_batch on the walkers' own residuals, with the dense factor (solver=None)
and with solver="auto" (sf_diagnose_banded_batch), for 128 walkers around the order's truth and for one.  Host time is in: the
methods return numpy arrays.  Beside them the device time of the calls alone, between events (sf_pointwise_batch,
sf_decompose_batch, and sf_diagnose_banded_batch asked for what each of the two returns).  The calls are timed in turn, ``reps``
calls each (default 5; one more in front is not timed), and the turn is repeated ``runs`` times (default 3): the medians over
the runs go into ONE JSON line, the last line printed.  Before the timing the two solvers' results are compared."""
import json
import statistics
import sys
import time

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
runs = int(sys.argv[3]) if len(sys.argv) > 3 else 3

import numpy as np  # noqa: E402
import torch  # noqa: E402
from _bench_common import timed  # noqa: E402

from starfish_amd import _device as D  # noqa: E402
from starfish_amd import _lib, synth  # noqa: E402

lib = _lib.require_gpu()
o = synth.make_order(N=N, m=4, seed=5)
model = synth.build_model(o)
walkers = {128: synth.walker_ball(o, B=128), 1: synth.walker_ball(o, B=128)[:1]}


def wall(call):
    """ms per call over ``reps`` calls (one more in front is not timed); the call returns host arrays."""
    call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


result = {"N": N, "reps": reps, "runs": runs, "unit": "ms per call, median over the runs"}
for B, P in walkers.items():
    dev, md, rows = model._pack(P, update_caches=False)
    hw = dev.halfwidth_bound(md, rows)
    W = int(hw.max())
    assert W <= dev.banded_window_halfwidth(), (W, dev.banded_window_halfwidth())
    dense, info_d = model.pointwise_batch(P, return_info=True)
    band, info_b = model.pointwise_batch(P, return_info=True, solver="auto")
    cd, cb = model.residual_components_batch(P), model.residual_components_batch(P, solver="auto")
    assert (info_d == 0).all() and (info_b == 0).all()
    print(f"N={N} B={B} half-width {W}: max |band - dense| / max |dense|: "
          + ", ".join(f"{key} {np.abs(band[key] - dense[key]).max() / np.abs(dense[key]).max():.3g}" for key in ("alpha", "loo_std", "z"))
          + "; components " + ", ".join(f"{key} {np.abs(cb[key] - cd[key]).max() / np.abs(cd[key]).max():.3g}"
                                         for key in ("emulator", "noise", "global", "local")), flush=True)
    with torch.cuda.device(dev.dev):
        Pd = D.to_dev(rows, dev.dev)
        n, ncomp = dev.n, 3 + int(md.n_local)
        alpha, cinv, cov, comp = (D.empty((B, 1, n), dev.dev), D.empty((B, n), dev.dev), D.empty((B, n), dev.dev),
                                  D.empty((B, ncomp, 1, n), dev.dev))
        info = D.empty((B,), dev.dev, torch.int32)
        ws = dev._reserve(max(dev.pointwise_workspace_bytes(md, B, 1), dev.decompose_workspace_bytes(md, B, 1),
                              dev.diagnose_banded_workspace_bytes(md, B, W, 1, True, True)))
        calls = {
            "pointwise_batch dense": lambda: model.pointwise_batch(P),
            "pointwise_batch auto": lambda: model.pointwise_batch(P, solver="auto"),
            "residual_components_batch dense": lambda: model.residual_components_batch(P),
            "residual_components_batch auto": lambda: model.residual_components_batch(P, solver="auto"),
        }
        device_calls = {
            "sf_pointwise_batch": lambda: dev._call("pointwise_batch", md, B, Pd, None, 1, n, 0, alpha, cinv, cov, None, info, ws=ws),
            "sf_diagnose_banded_batch (alpha, cinv_diag, cov_diag)": lambda: dev._call(
                "diagnose_banded_batch", md, B, Pd, W, None, 1, n, 0, alpha, cinv, cov, None, None, info, ws=ws),
            "sf_decompose_batch": lambda: dev._call("decompose_batch", md, B, Pd, None, 1, n, 0, comp, alpha, None, info, ws=ws),
            "sf_diagnose_banded_batch (alpha, comp)": lambda: dev._call(
                "diagnose_banded_batch", md, B, Pd, W, None, 1, n, 0, alpha, None, None, comp, None, info, ws=ws),
        }
        times = {name: [] for name in list(calls) + list(device_calls)}
        for _ in range(runs):
            for name, call in calls.items():
                times[name].append(wall(call))
            for name, call in device_calls.items():
                times[name].append(timed(call, reps))
                assert int(info.abs().max()) == 0
        del ws
    for name, v in times.items():
        result[f"B={B} {name}"] = round(statistics.median(v), 3)
        print(f"N={N} B={B} {name}: {statistics.median(v):9.3f} ms per call (median of {runs} runs of {reps} calls; "
              f"{min(v):.3f} .. {max(v):.3f})", flush=True)
    dev.release_workspace()
print(json.dumps(result), flush=True)
