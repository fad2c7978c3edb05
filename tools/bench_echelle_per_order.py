"""ms per EchelleModel.log_likelihood_batch with per-order nuisance parameters (host packing, copies and the
synchronisation included), 25 orders x 3000 px x 64 walkers by default:

  (a) shared       every parameter shared (synth.build_echelle: the cfg-3 model)
  (b) per-order    cheb / log_scale / global_cov / local_cov per order, one row layout (1 local kernel each)
  (c) mixed        as (b) with 0-3 local kernels per order: one multi-order call with one descriptor per order
  (d) grouped      (c) split into one multi-order call per row layout (what the one pass replaces)

Every case starts from released workspaces (each model's lead order keeps the workspace of its multi-order calls:
~120 GB at this size), and the line reports the C-ABI calls one evaluation made.

python tools/bench_echelle_per_order.py [orders] [npix] [walkers] [repeats]"""
import gc
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from starfish_amd import _device as D  # noqa: E402
from starfish_amd import _multi  # noqa: E402
from starfish_amd import synth  # noqa: E402
from starfish_amd.models import EchelleModel  # noqa: E402

n_orders = int(sys.argv[1]) if len(sys.argv) > 1 else 25
N = int(sys.argv[2]) if len(sys.argv) > 2 else 3000
B = int(sys.argv[3]) if len(sys.argv) > 3 else 64
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 10
PER = ["cheb", "log_scale", "global_cov", "local_cov"]


def per_order_model(orders, n_local):
    models = []
    for i, o in enumerate(orders):
        c = dict(synth.centre_params(o))
        w = o["wave"]
        nl = n_local(i)
        c["local_cov"] = [dict(mu=float(w[(k + 1) * len(w) // (nl + 1)]), log_amp=-8.0, log_sigma=float(np.log(15.0)))
                          for k in range(nl)]
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


def grouped(em, P):
    """(d) the way a multi-order call had to be split before per-segment descriptors: one call per row layout."""
    _, cols = em._layout()
    packed = [m._pack(P[:, c], update_caches=False) for m, c in zip(em.orders, cols)]
    groups = {}
    for idx, (dev, md, rows) in enumerate(packed):
        groups.setdefault((str(dev.dev),) + D.model_desc_key(md), []).append(idx)
    plans = [(idxs, D.loglike_multi([packed[i][0] for i in idxs], packed[idxs[0]][1], [packed[i][2] for i in idxs],
                                    sync=False)) for idxs in groups.values()]
    vals = np.zeros((len(em.orders), B))
    for idxs, plan in plans:
        for i, out in zip(idxs, plan.collect()):
            vals[i] = out["lnl"]
    return vals.sum(axis=0), len(groups)


calls = []  # len(plan.calls) of every MultiPlan built


class CountingPlan(D.MultiPlan):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        calls.append(len(self.calls))


_multi.MultiPlan = CountingPlan


def release(*models):
    import torch

    for em in models:
        for m in em.orders:
            m._device().release_workspace()
    gc.collect()
    torch.cuda.empty_cache()


def timed(fn):
    release(shared, one, mixed)  # (nothing of an earlier case holds HBM)
    for _ in range(2):
        out = fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        del calls[:]
        fn()
    ms = (time.perf_counter() - t0) / reps * 1e3
    return ms, out, sum(calls)


orders = synth.make_echelle(n_orders, N)
shared = synth.build_echelle(orders)
P_shared = synth.shared_ball(orders[0], B=B, seed=1)
one = per_order_model(orders, lambda i: 1)
mixed = per_order_model(orders, lambda i: i % 4)
P_one, P_mixed = ball(one), ball(mixed)

res, vals = {}, {}
cases = (("a_shared", lambda: shared.log_likelihood_batch(P_shared)),
         ("b_per_order", lambda: one.log_likelihood_batch(P_one)),
         ("c_mixed_one_pass", lambda: mixed.log_likelihood_batch(P_mixed)),
         ("d_mixed_grouped", lambda: grouped(mixed, P_mixed)[0]))
for name, fn in cases:
    ms, vals[name], n_calls = timed(fn)
    res[name + "_ms"], res[name + "_calls"] = ms, n_calls
    assert np.isfinite(vals[name]).all(), name
release(shared, one, mixed)
np.testing.assert_allclose(vals["d_mixed_grouped"], vals["c_mixed_one_pass"], rtol=1e-10)  # the same values either way
res.update(orders=n_orders, npix=N, walkers=B, repeats=reps, labels_b=len(one.labels), labels_c=len(mixed.labels),
           c_layouts=len({D.model_desc_key(m._model_desc(m._device())) for m in mixed.orders}))
for name, _ in cases:
    print(f"{name:>18}: {res[name + '_ms']:8.1f} ms per call, {res[name + '_calls']} C-ABI call(s)")
print(json.dumps(res))
