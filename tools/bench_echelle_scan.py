"""ms per call of the score scan for new local kernels of an EchelleModel on the band solver (host packing, copies and the
synchronisation included), for the model of tools/bench_echelle_fisher.py (orders sampling cheb / log_scale / global_cov /
local_cov on their own with 0-3 local kernels, m = 8), 25 orders x 3000 px by default, every pixel x 3 widths per order, at one
walker (the MAP point) and at 8:

  (a) one pass         EchelleModel.local_kernel_scan_batch(P, solver="auto"): sf_local_scan_banded_multi_batch_md
  (b) per-order loop   every order's SpectrumModel.local_kernel_scan_batch(P[:, cols], solver="auto"): the same kernels one order
                       at a time (what there was before the one pass)
  (c) proposal         EchelleModel.propose_local_kernels(P=P, solver="auto"): (a) with the means over the walkers taken on the
                       device (sf_local_scan_mean) and the peak picking per order
  (d) device side of (a)   enqueue() + collect() of a BandedMultiScanPlan built once: launches, copies, synchronisation
  (e) device side of (b)   every order's sf_local_scan_banded_batch through DeviceOrder, one after the other
(a) - (c) include the host's checks of the candidates -- the patch of every candidate, a Python loop
(starfish_amd._device.local_scan_patches) that both (a) and (b) run twice per order; (d) and (e) leave them out.

The five alternate in one process: every round times one call of each, after two untimed calls of each; the median and the
range over the rounds (5 by default) are reported, and the largest difference of (a) against (b) over the largest number of its
kind.  No threshold is attached: the candidate kernel is shared by (a) and (b) and dominates both.

python tools/bench_echelle_scan.py [orders] [npix] [rounds] [walkers ...]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from starfish_amd import _device as D  # noqa: E402
from starfish_amd import synth  # noqa: E402
from starfish_amd.models import EchelleModel  # noqa: E402

n_orders = int(sys.argv[1]) if len(sys.argv) > 1 else 25
N = int(sys.argv[2]) if len(sys.argv) > 2 else 3000
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
walkers = [int(v) for v in sys.argv[4:]] or [1, 8]
PER = ["cheb", "log_scale", "global_cov", "local_cov"]
SIGMAS = (8.0, 15.0, 30.0)


def per_order_model(orders):
    models = []
    for i, o in enumerate(orders):
        c = dict(synth.centre_params(o))
        w = o["wave"]
        nl = i % 4
        c["local_cov"] = [dict(mu=float(w[(k + 1) * len(w) // (nl + 1)] + 0.37 * (w[1] - w[0])), log_amp=-8.0,
                               log_sigma=float(np.log(15.0))) for k in range(nl)]
        if not nl:
            del c["local_cov"]
        models.append(synth.build_model(o, params=c))
    return EchelleModel.from_orders(models, per_order=PER)


def ball(em, B, seed=1):
    rng = np.random.default_rng(seed)
    p0 = em.get_param_vector()
    scale = []
    for k in em.labels:
        key = k.split(":", 1)[1] if k.startswith("order") else k
        if key.startswith("local_cov:"):
            key = "local_cov:0:" + key.split(":")[2]
        scale.append(synth._BALL[key])
    return p0[None, :] + np.array(scale)[None, :] * rng.standard_normal((B, len(p0)))


def spread(values):
    return dict(median=float(np.median(values)), min=float(np.min(values)), max=float(np.max(values)))


orders = synth.make_echelle(n_orders, N)
em = per_order_model(orders)
_, cols = em._layout()
res = dict(orders=n_orders, npix=N, rounds=rounds, m=int(em.orders[0]._pack(None, update_caches=False)[0].m), sigmas=SIGMAS,
           candidates_per_order=len(SIGMAS) * N, sizes={})
for B in walkers:
    P = ball(em, B)
    cases = {"a_one_pass": lambda: em.local_kernel_scan_batch(P, sigmas=SIGMAS, return_info=True, solver="auto"),
             "b_per_order_loop": lambda: [m.local_kernel_scan_batch(P[:, c], sigmas=SIGMAS, return_info=True, solver="auto")
                                          for m, c in zip(em.orders, cols)],
             "c_proposal": lambda: em.propose_local_kernels(P=P, sigmas=SIGMAS, solver="auto")}
    packed = [m._pack(P[:, c], update_caches=False) for m, c in zip(em.orders, cols)]
    cands = [np.array([(mu, s) for s in SIGMAS for mu in np.asarray(m.data.wave)]) for m in em.orders]
    plan = D.BandedMultiScanPlan([p[0] for p in packed], [p[1] for p in packed], [p[2] for p in packed], cands, solver="auto")
    assert all(f.all() for f in plan.fits)  # (every unit on the band kernels)

    def device_side_one_pass():
        plan.enqueue()
        return plan.collect()

    def device_side_loop():
        return [dev._local_scan_call("local_scan_banded_batch", md, rows, cand, None, dev.local_scan_banded_workspace_bytes)
                for (dev, md, rows), cand in zip(packed, cands)]

    cases["d_device_side_of_a"], cases["e_device_side_of_b"] = device_side_one_pass, device_side_loop
    out = {}
    for key, fn in cases.items():
        for _ in range(2):
            out[key] = fn()
    runs = {key: [] for key in cases}
    for _ in range(rounds):
        for key, fn in cases.items():
            t0 = time.perf_counter()
            fn()
            runs[key].append((time.perf_counter() - t0) * 1e3)
    r = {key + "_ms": spread(v) for key, v in runs.items()}
    (ra, info), rb = out["a_one_pass"], out["b_per_order_loop"]
    assert (info == 0).all() and all((i == 0).all() for _, i in rb)
    diff = 0.0
    for a, (b, _) in zip(ra, rb):
        for key in ("quad", "trace", "information"):
            assert np.isfinite(a[key]).all()
            diff = max(diff, float(np.abs(a[key] - b[key]).max() / np.abs(b[key]).max()))
    r["largest_difference_of_a_and_b"] = diff
    r["proposed"] = int(sum(len(v) for v in out["c_proposal"]))
    for one, each in zip(out["d_device_side_of_a"], out["e_device_side_of_b"]):
        assert all(np.array_equal(one[key], each[key]) for key in ("quad", "trace", "fisher", "info"))
    a, b = r["a_one_pass_ms"], r["b_per_order_loop_ms"]
    r["b_over_a"], r["c_over_a"] = b["median"] / a["median"], r["c_proposal_ms"]["median"] / a["median"]
    r["e_over_d"] = r["e_device_side_of_b_ms"]["median"] / r["d_device_side_of_a_ms"]["median"]
    res["sizes"][str(B)] = r
    print(f"{B} walker(s), {n_orders * B} units, {len(SIGMAS) * N} candidates per order:")
    for key in cases:
        v = r[key + "_ms"]
        print(f"{key:>22}: {v['median']:9.2f} ms per call (median of {rounds}; range {v['min']:.2f} .. {v['max']:.2f})")
    print(f"{'b / a, c / a, e / d':>22}: {r['b_over_a']:.2f}, {r['c_over_a']:.2f}, {r['e_over_d']:.2f}; largest |a - b| / largest {diff:.3g}; "
          f"{r['proposed']} kernels proposed")
print(json.dumps(res))
