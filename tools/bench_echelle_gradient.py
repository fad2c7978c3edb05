"""ms per call of the multi-order likelihood and its gradient (host packing, copies and the synchronisation included), for an
EchelleModel whose orders sample cheb / log_scale / global_cov / local_cov on their own with 0-3 local kernels, 25 orders x
3000 px x 64 walkers by default (the cfg-3 shape):

  (a) likelihood   EchelleModel.log_likelihood_batch: sf_loglike_multi_batch_md, one factorisation per unit
  (b) one pass     EchelleModel.log_likelihood_gradient_batch: sf_loglike_multi_grad_batch_md, one factorisation per unit, and
                   the sum over the orders on the device
  (c) per order    the loop over every order's SpectrumModel.log_likelihood_full_gradient_batch: two calls and two
                   factorisations per order, the sum over the orders on the host (what there was before the one pass)

Every case starts from released workspaces; the gradient cases run interleaved (c) | (b) | (c) in one process.  For (a) and
(b) the library's stage times of one call are printed too (transform chains, fills, factorisation, logdet / finish: the
rest of (b) is the solve of the staging area, the inverse factor, the contractions and the host), and the contraction launches
alone, summed over the orders, through the timing aids of the single-order gradient calls.

python tools/bench_echelle_gradient.py [orders] [npix] [walkers] [repeats]"""
import ctypes as C
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
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
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
    """(c): every order's own full gradient, summed over the orders in ascending index on the host."""
    labels, cols, _, _ = em._gradient_layout()
    lnl, grad = None, np.zeros((len(P), len(labels)))
    seen = np.zeros(len(labels), dtype=bool)
    for m, c in zip(em.orders, cols):
        l, g = m.log_likelihood_full_gradient_batch(P[:, c])
        lnl = l if lnl is None else lnl + l
        grad[:, c] = np.where(seen[c][None, :], grad[:, c] + g, g)
        seen[c] = True
    return lnl, grad


def contraction_stage(em, P):
    """ms of the contraction launches alone, summed over the orders: per order the launches of sf_launch_cov_grad and of
    sf_launch_mean_grad on the workspace its own single-order gradient call left (the library's two timing aids).  These are
    the launches the one pass makes per segment."""
    import torch

    from starfish_amd import _device as D

    _, cols, requests, _ = em._gradient_layout()
    cov_ms = mean_ms = 0.0
    for m, c, (columns, want_cov) in zip(em.orders, cols, requests):
        dev, md, rows = m._pack(P[:, c], update_caches=False)
        with torch.cuda.device(dev.dev):
            Pd, nb = D.to_dev(rows, dev.dev), len(rows)
            lnl, info = D.empty((nb,), dev.dev), D.empty((nb,), dev.dev, torch.int32)
            grad = D.empty((nb, 32), dev.dev)
            h = (C.c_int * len(columns))(*columns)
            runs = [("loglike_mean_grad_batch", "debug_loglike_mean_grad_contract", dev.loglike_mean_grad_workspace_bytes(md, nb, len(columns)),
                     (h, len(columns)))]
            if want_cov:
                runs.append(("loglike_grad_batch", "debug_loglike_grad_contract", dev.loglike_grad_workspace_bytes(md, nb), ()))
            for whole, part, nbytes, lead in runs:
                ws = dev._reserve(nbytes)
                dev._call(whole, md, nb, Pd, *lead, lnl, grad, 32, None, info, ws=ws)
                dev._call(part, md, nb, Pd, *lead, grad, 32, ws=ws)
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                dev._call(part, md, nb, Pd, *lead, grad, 32, ws=ws)
                t1.record()
                torch.cuda.synchronize()
                if lead:
                    mean_ms += t0.elapsed_time(t1)
                else:
                    cov_ms += t0.elapsed_time(t1)
            dev.release_workspace()
    return dict(cov_contractions=cov_ms, mean_contractions=mean_ms)


def release(em):
    import torch

    for m in em.orders:
        m._device().release_workspace()
    gc.collect()
    torch.cuda.empty_cache()


def timed(em, fn, stages=False):
    import torch

    release(em)  # (nothing of an earlier case holds HBM)
    for _ in range(2):
        out = fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    ms = (time.perf_counter() - t0) / reps * 1e3
    prof = None
    if stages:
        lib = em.orders[0]._device().lib
        torch.cuda.synchronize()
        lib.sf_profile_read(None, None, None, None)
        lib.sf_profile_enable(1)
        fn()
        torch.cuda.synchronize()
        lib.sf_profile_enable(0)
        acc = (C.c_double * 6)()
        lib.sf_profile_read(acc, None, None, None)
        prof = dict(zip(("transform", "fill", "potrf", "solve"), (acc[0], acc[1], acc[3], acc[4])))
    return ms, out, prof


orders = synth.make_echelle(n_orders, N)
em = per_order_model(orders)
P = ball(em)
res = dict(orders=n_orders, npix=N, walkers=B, repeats=reps, labels=len(em.labels))
res["a_likelihood_ms"], lnl_a, res["a_stages_ms"] = timed(em, lambda: em.log_likelihood_batch(P), stages=True)
res["c_per_order_ms_first"], (lnl_c, grad_c), _ = timed(em, lambda: per_order_loop(em, P))
res["b_one_pass_ms"], (lnl_b, grad_b), res["b_stages_ms"] = timed(em, lambda: em.log_likelihood_gradient_batch(P), stages=True)
res["c_per_order_ms_second"], _, _ = timed(em, lambda: per_order_loop(em, P))
release(em)
res["contraction_launches_ms"] = contraction_stage(em, P)
release(em)
assert np.isfinite(lnl_b).all() and np.isfinite(grad_b).all()
np.testing.assert_allclose(lnl_b, lnl_a, rtol=1e-13)
np.testing.assert_allclose(lnl_c, lnl_b, rtol=1e-12)
scale = np.abs(grad_c).max(axis=0) + 1e-300
res["largest_difference_of_b_and_c"] = float((np.abs(grad_b - grad_c) / scale[None, :]).max())
for key in ("a_likelihood_ms", "c_per_order_ms_first", "b_one_pass_ms", "c_per_order_ms_second"):
    print(f"{key:>24}: {res[key]:9.1f} ms per call")
for key in ("a_stages_ms", "b_stages_ms"):
    print(f"{key:>24}: " + ", ".join(f"{k} {v:.1f}" for k, v in res[key].items()))
print(f"{'contraction launches':>24}: " + ", ".join(f"{k} {v:.2f} ms" for k, v in res["contraction_launches_ms"].items())
      + f" over the {n_orders} orders")
print(json.dumps(res))
