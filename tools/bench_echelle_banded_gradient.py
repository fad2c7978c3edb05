"""ms per call of the multi-order likelihood and its gradient on the band solver (host packing, copies and the synchronisation
included), for the EchelleModel of tools/bench_echelle_gradient.py (orders sampling cheb / log_scale / global_cov / local_cov on
their own with 0-3 local kernels), 25 orders x 3000 px x 64 walkers by default (the cfg-3 shape); walkers = 1 is one train() step:

  (a) dense one pass    EchelleModel.log_likelihood_gradient_batch(P): sf_loglike_multi_grad_batch_md
  (b) per-order loop    every order's SpectrumModel.log_likelihood_full_gradient_batch(P[:, cols], solver="auto",
                        covariance_solver="auto"), the sum over the orders on the host: the band kernels one order at a time
                        (what there was before the one pass on the band solver: the baseline)
  (c) banded one pass   EchelleModel.log_likelihood_gradient_batch(P, solver="auto"): sf_loglike_banded_multi_grad_batch_md

(a) is timed once (mean of 3 calls after 2).  (b) and (c) alternate in one process, `repeats` rounds (at least 5); every round
starts each case from released workspaces, runs it twice untimed and times the mean of 3 calls.  Median and range over the
rounds are reported, the largest column difference of (c) against (a) over the column's largest entry, and how many units the
band kernels took.

python tools/bench_echelle_banded_gradient.py [orders] [npix] [walkers] [repeats]"""
import gc
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from starfish_amd import synth  # noqa: E402
from starfish_amd.models import EchelleModel  # noqa: E402

n_orders = int(sys.argv[1]) if len(sys.argv) > 1 else 25
N = int(sys.argv[2]) if len(sys.argv) > 2 else 3000
B = int(sys.argv[3]) if len(sys.argv) > 3 else 64
reps = max(int(sys.argv[4]) if len(sys.argv) > 4 else 5, 5)
PER = ["cheb", "log_scale", "global_cov", "local_cov"]
CALLS = 3


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


def ball(em, seed=1):
    rng = np.random.default_rng(seed)
    p0 = em.get_param_vector()
    scale = []
    for k in em.labels:
        key = k.split(":", 1)[1] if k.startswith("order") else k
        if key.startswith("local_cov:"):
            key = "local_cov:0:" + key.split(":")[2]
        scale.append(synth._BALL[key])
    return p0[None, :] + np.array(scale)[None, :] * rng.standard_normal((B, len(p0)))


def per_order_loop(em, P):
    """(b): every order's own full gradient on the band solver, summed over the orders in ascending index on the host."""
    labels, cols, _, _ = em._gradient_layout()
    lnl, grad = None, np.zeros((len(P), len(labels)))
    seen = np.zeros(len(labels), dtype=bool)
    for m, c in zip(em.orders, cols):
        l, g = m.log_likelihood_full_gradient_batch(P[:, c], solver="auto", covariance_solver="auto")
        lnl = l if lnl is None else lnl + l
        grad[:, c] = np.where(seen[c][None, :], grad[:, c] + g, g)
        seen[c] = True
    return lnl, grad


def release(em):
    import torch

    for m in em.orders:
        m._device().release_workspace()
    gc.collect()
    torch.cuda.empty_cache()


def timed(em, fn):
    release(em)  # (nothing of an earlier case holds HBM)
    for _ in range(2):
        out = fn()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        fn()
    return (time.perf_counter() - t0) / CALLS * 1e3, out


def spread(values):
    return dict(median=float(np.median(values)), min=float(np.min(values)), max=float(np.max(values)), runs=[float(v) for v in values])


orders = synth.make_echelle(n_orders, N)
em = per_order_model(orders)
P = ball(em)
res = dict(orders=n_orders, npix=N, walkers=B, rounds=reps, calls_per_round=CALLS, labels=len(em.labels))
_, cols, _, _ = em._gradient_layout()
taken = widest = 0
for m, c in zip(em.orders, cols):
    dev, md, rows = m._pack(P[:, c], update_caches=False)
    hw = dev.halfwidth_bound(md, rows)
    taken += int(np.count_nonzero(hw <= dev.banded_window_halfwidth()))
    widest = max(widest, int(hw[hw <= dev.banded_window_halfwidth()].max(initial=0)))
res["units"], res["units_on_the_band_kernels"], res["largest_halfwidth_bound_of_them"] = n_orders * B, taken, widest
res["a_dense_one_pass_ms"], (lnl_a, grad_a) = timed(em, lambda: em.log_likelihood_gradient_batch(P))
runs_b, runs_c = [], []
for _ in range(reps):
    ms, (lnl_b, grad_b) = timed(em, lambda: per_order_loop(em, P))
    runs_b.append(ms)
    ms, (lnl_c, grad_c) = timed(em, lambda: em.log_likelihood_gradient_batch(P, solver="auto"))
    runs_c.append(ms)
release(em)
res["b_per_order_loop_ms"], res["c_banded_one_pass_ms"] = spread(runs_b), spread(runs_c)
assert np.isfinite(lnl_c).all() and np.isfinite(grad_c).all()
np.testing.assert_allclose(lnl_c, lnl_a, rtol=1e-8)
np.testing.assert_allclose(lnl_b, lnl_c, rtol=1e-8)
scale = np.abs(grad_a).max(axis=0) + 1e-300
res["largest_difference_of_c_and_a"] = float((np.abs(grad_c - grad_a) / scale[None, :]).max())
res["largest_difference_of_c_and_b"] = float((np.abs(grad_c - grad_b) / scale[None, :]).max())
b, c = res["b_per_order_loop_ms"], res["c_banded_one_pass_ms"]
res["c_faster_than_b_beyond_the_spread"] = bool(c["max"] < b["min"])
res["a_over_c"], res["b_over_c"] = res["a_dense_one_pass_ms"] / c["median"], b["median"] / c["median"]
print(f"{'a dense one pass':>22}: {res['a_dense_one_pass_ms']:9.2f} ms per call")
for key, v in (("b per-order loop", b), ("c banded one pass", c)):
    print(f"{key:>22}: {v['median']:9.2f} ms per call (median of {reps} rounds; range {v['min']:.2f} .. {v['max']:.2f})")
print(f"{'a / c, b / c':>22}: {res['a_over_c']:.2f}, {res['b_over_c']:.2f}; c faster than b beyond the spread: "
      f"{res['c_faster_than_b_beyond_the_spread']}")
print(f"{'c against a':>22}: largest column difference / largest entry {res['largest_difference_of_c_and_a']:.3g}; "
      f"{taken} of {n_orders * B} units on the band kernels (largest bound {widest})")
print(json.dumps(res))
