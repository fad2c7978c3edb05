"""ms per call of the Fisher information of an EchelleModel in its mean-flux parameters on the band solver (host packing, copies
and the synchronisation included), for the model of tools/bench_echelle_banded_gradient.py (orders sampling cheb / log_scale /
global_cov / local_cov on their own with 0-3 local kernels: 8 mean columns per order), 25 orders x 3000 px by default, at one
walker (the MAP point, where the matrix is asked for) and at 64:

  (a) one pass         EchelleModel.fisher_information_batch(P, solver="auto"): sf_fisher_banded_multi_batch_md and
                       sf_multi_fisher_reduce
  (b) per-order loop   every order's SpectrumModel.fisher_information_batch(P[:, cols], solver="auto"), then
                       reduce_fisher_host: the band kernels one order at a time (what there was before the one pass)
  (c) gradient         EchelleModel.log_likelihood_gradient_batch(P, solver="auto"), as the scale

The three alternate in one process: every round times one call of each, after two untimed calls of each; the median and the
range over the rounds (at least 20) are reported, the largest difference of (a) against (b) over sqrt(F_ii F_jj), and how many
units the band kernels took.

python tools/bench_echelle_fisher.py [orders] [npix] [rounds] [walkers ...]"""
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
rounds = max(int(sys.argv[3]) if len(sys.argv) > 3 else 20, 20)
walkers = [int(v) for v in sys.argv[4:]] or [1, 64]
PER = ["cheb", "log_scale", "global_cov", "local_cov"]


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


def per_order_loop(em, P, cols, sources):
    """(b): every order's own call on the band solver, then the order sum on the host."""
    units = [m.fisher_information_batch(P[:, c], return_info=True, solver="auto") for m, c in zip(em.orders, cols)]
    zeros = np.zeros((len(units), len(P)))
    return D.reduce_fisher_host(zeros, np.stack([info for _, info in units]), [F for F, _ in units], sources)[1]


def spread(values):
    return dict(median=float(np.median(values)), min=float(np.min(values)), max=float(np.max(values)))


orders = synth.make_echelle(n_orders, N)
em = per_order_model(orders)
_, cols, columns, sources = em._fisher_layout("auto")
res = dict(orders=n_orders, npix=N, rounds=rounds, labels=len(em.labels), fisher_labels=len(em.mean_gradient_labels),
           columns_per_order=sorted(set(len(c) for c in columns)), sizes={})
for B in walkers:
    P = ball(em, B)
    cases = {"a_one_pass": lambda: em.fisher_information_batch(P, solver="auto"),
             "b_per_order_loop": lambda: per_order_loop(em, P, cols, sources),
             "c_gradient": lambda: em.log_likelihood_gradient_batch(P, solver="auto")}
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
    Fa, Fb = out["a_one_pass"], out["b_per_order_loop"]
    assert np.isfinite(Fa).all() and np.array_equal(Fa, Fa.transpose(0, 2, 1))
    d = np.sqrt(np.einsum("bii->bi", Fa))
    r["largest_difference_of_a_and_b"] = float((np.abs(Fa - Fb) / (d[:, :, None] * d[:, None, :])).max())
    plan = D.BandedMultiFisherPlan(*([m._pack(P[:, c], update_caches=False)[k] for m, c in zip(em.orders, cols)] for k in range(3)),
                                   columns, solver="auto")
    r["units"], r["units_on_the_band_kernels"], r["halfwidth"] = plan.units, int(sum(f.sum() for f in plan.fits)), plan.halfwidth
    a, b = r["a_one_pass_ms"], r["b_per_order_loop_ms"]
    r["b_over_a"], r["a_over_c"] = b["median"] / a["median"], a["median"] / r["c_gradient_ms"]["median"]
    r["a_not_slower_than_b_by_more_than_5_percent"] = bool(a["median"] <= 1.05 * b["median"])
    res["sizes"][str(B)] = r
    print(f"{B} walker(s), {plan.units} units ({r['units_on_the_band_kernels']} on the band kernels, half-width {plan.halfwidth}):")
    for key in cases:
        v = r[key + "_ms"]
        print(f"{key:>20}: {v['median']:9.2f} ms per call (median of {rounds}; range {v['min']:.2f} .. {v['max']:.2f})")
    print(f"{'b / a, a / c':>20}: {r['b_over_a']:.2f}, {r['a_over_c']:.2f}; largest |a - b| / sqrt(F_ii F_jj) "
          f"{r['largest_difference_of_a_and_b']:.3g}")
print(json.dumps(res))
