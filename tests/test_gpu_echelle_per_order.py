"""EchelleModel with per-order nuisance parameters on the device: orders with their own Chebyshev terms, log_scale,
global kernel and 0, 1 or 3 local kernels (different C-ABI row strides) in ONE multi-order call
(sf_loglike_multi_batch_md), checked order by order against the CPU oracle; and the C-ABI entry point with one
descriptor per segment against the single-descriptor one.  Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest

from gpu_helpers import device_order, oracle_order, pack_rows
from oracle import sf_oracle as O
from per_order_cases import PER, ball, oracle_params, per_order_models
from starfish_amd import _device as D
from starfish_amd import _lib, _multi, samplers, synth
from starfish_amd.models import EchelleModel

import transform_cases as TC

pytestmark = pytest.mark.gpu

N_LOCAL = (0, 1, 3, 1, 0)
SIZES = (256, 320, 192, 288, 224)


def close(a, b, rtol=1e-8):
    return np.all(np.abs(np.asarray(a) - np.asarray(b)) <= rtol * np.abs(b) + 1e-8)


@pytest.fixture(scope="module")
def model():
    orders, models = per_order_models(N_LOCAL, sizes=list(SIZES), m=4, seed0=80)
    em = EchelleModel.from_orders(models, per_order=PER)
    return orders, models, em


def count_plans(monkeypatch):
    plans = []
    real = D.MultiPlan

    class Counting(real):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            plans.append(self)

    monkeypatch.setattr(_multi, "MultiPlan", Counting)
    return plans


def test_per_order_batch_vs_oracle_in_one_pass(model, monkeypatch):
    orders, models, em = model
    strides = {m._pack(None, update_caches=False)[2].shape[1] for m in models}
    assert len(strides) == 3  # really different row layouts
    P = ball(em, B=5, seed=4)
    _, cols = em._layout()
    assert len({tuple(P[0, c]) for c in cols}) == len(models)  # every order sees its own values
    plans = count_plans(monkeypatch)
    total, info, per_order = em.log_likelihood_batch(P, return_info=True, return_orders=True)
    assert len(plans) == 1 and plans[0].per_order and len(plans[0].calls) == 1
    assert (info == 0).all()
    for i, (o, m) in enumerate(zip(orders, models)):
        oo = oracle_order(o)
        for b in range(len(P)):
            want = O.log_likelihood(oo, oracle_params(m, P[b, cols[i]]))
            assert close(per_order[i, b], want), (i, b, per_order[i, b], want)
    np.testing.assert_allclose(total, per_order.sum(axis=0), rtol=1e-14)
    # each order's own batched pass gives the same values
    for i, m in enumerate(models):
        np.testing.assert_allclose(per_order[i], m.log_likelihood_batch(P[:, cols[i]]), rtol=1e-12)
    # the scalar API: the sum over orders at one walker
    em.set_param_vector(P[1])
    assert close(em.log_likelihood(), per_order[:, 1].sum())


def test_out_of_grid_walker_and_structured_solver(model):
    _, models, em = model
    labels = em.labels
    P = ball(em, B=6, seed=7)
    dense, info = em.log_likelihood_batch(P, return_info=True)
    P2 = P.copy()
    P2[2, labels.index("T")] = 9000.0
    t2, info2 = em.log_likelihood_batch(P2, return_info=True)
    assert t2[2] == -np.inf and info2[2] == -1
    keep = [0, 1, 3, 4, 5]
    np.testing.assert_allclose(t2[keep], dense[keep], rtol=1e-12)
    assert (info2[keep] == 0).all()
    try:
        for m in models:
            m.solver = "auto"
        auto, info_a, per_a = em.log_likelihood_batch(P2, return_info=True, return_orders=True)
    finally:
        for m in models:
            m.solver = "dense"
    np.testing.assert_allclose(auto[keep], dense[keep], rtol=1e-10)
    assert auto[2] == -np.inf and info_a[2] == -1 and (info_a[keep] == 0).all()


def test_ensemble_sampler_runs_on_per_order_batches(model):
    _, _, em = model
    ndim = len(em.labels)
    nwalkers = 2 * ndim
    p0 = ball(em, B=nwalkers, seed=11)
    sampler = samplers.EnsembleSampler(nwalkers, ndim, em.log_likelihood_batch, seed=3)
    x, lp = sampler.run_mcmc(p0, 3)
    assert x.shape == (nwalkers, ndim) and np.isfinite(lp).all()
    assert np.isfinite(sampler.get_log_prob()).all()


def _segments(devs, rows_dev):
    segs = (_lib.Segment * len(devs))()
    for k, (d, r) in enumerate(zip(devs, rows_dev)):
        segs[k] = _lib.Segment(d.ctx, D.ptr(r).value, int(r.shape[0]), 0)
    return segs


def test_md_entry_point_with_one_descriptor_repeated_is_bit_identical():
    """cfg-3-style orders (N = 3000, m = 8, shared parameters): the per-segment entry point given the same descriptor
    for every segment gives the bits of sf_loglike_multi_batch, with the same workspace size."""
    orders = synth.make_echelle(6, 3000)
    em = synth.build_echelle(orders)
    P = synth.shared_ball(orders[0], B=8, seed=5)
    packed = [m._pack(P, update_caches=False) for m in em.orders]
    devs, md, rows = [p[0] for p in packed], packed[0][1], [p[2] for p in packed]
    one = D.MultiPlan(devs, md, rows)
    many = D.MultiPlan(devs, [md] * len(devs), rows)
    assert not one.per_order and many.per_order
    lib = devs[0].lib
    segs = _segments(devs, one.P)
    assert lib.sf_multi_workspace_bytes(segs, len(devs), C.byref(md)) == \
        lib.sf_multi_workspace_bytes_md(segs, len(devs), D.MultiPlan._desc_array([md] * len(devs)))
    one.enqueue()
    a = one.collect()
    many.enqueue()
    b = many.collect()
    for x, y in zip(a, b):
        assert (x["info"] == 0).all()
        for key in ("lnl", "logdet", "sqmah", "log_scale", "info"):
            np.testing.assert_array_equal(x[key], y[key])


def test_md_entry_point_refuses_a_vsini_segment_outside_the_fft_limits():
    """A segment whose descriptor has vsini on an order with nf = 8 is refused up front (SF_EINVAL, the error names
    the segment), although segment 0's descriptor has no vsini."""
    import torch

    good_o = TC.make_nf_order(64, seed=5)
    small = synth.make_order(N=6, m=4, seed=3, pad=0.04)
    do_good, do_small = device_order(oracle_order(good_o)), device_order(oracle_order(small))
    assert do_small.nf == 8
    plist = TC.walkers(2, log_scale=True)
    noflat = [dict(p) for p in plist]
    for p in noflat:
        del p["vsini"]
    md_good, rows_good = pack_rows(do_good, noflat)
    md_bad = do_small.model_desc(True, True, True, False, 0, 2)
    rows_bad = np.zeros((2, 6 + do_small.P + 2))
    lib = do_good.lib
    with torch.cuda.device(do_good.dev):
        r = [D.to_dev(rows_good, do_good.dev), D.to_dev(rows_bad, do_good.dev)]
        segs = _segments([do_good, do_small], r)
        models = D.MultiPlan._desc_array([md_good, md_bad])
        assert lib.sf_multi_workspace_bytes_md(segs, 2, models) == 0
        out = D.empty((4,), do_good.dev)
        info = D.empty((4,), do_good.dev, torch.int32)
        ws = D.workspace(1 << 20, do_good.dev)
        rc = lib.sf_loglike_multi_batch_md(segs, 2, models, D.ptr(out), None, None, None, D.ptr(info), D.ptr(ws),
                                           ws.numel(), D.stream_ptr(do_good.dev))
        assert rc == -1  # SF_EINVAL
        err = lib.sf_last_error().decode()
        assert "segment 1" in err and "16 <= nf <= 65536" in err, err
        # the same segments with a descriptor that has no vsini are accepted
        md_ok = do_small.model_desc(False, True, True, False, 0, 2)
        assert lib.sf_multi_workspace_bytes_md(segs, 2, D.MultiPlan._desc_array([md_good, md_ok])) > 0
    do_small.release_workspace()


def test_vsini_on_later_orders_only_vs_oracle(monkeypatch):
    """Order 0 is not broadened, the later orders sample their own vsini: the broadening buffers of the one call
    exist only because of later segments (they are sized for the union of the descriptors)."""
    orders, models = per_order_models((1, 0, 3), sizes=[256, 224, 288], m=4, seed0=90, no_vsini=(0,))
    em = EchelleModel.from_orders(models, per_order=PER + ("vsini",))
    labels = em.labels
    assert "vsini" not in labels and "order0:vsini" not in labels and "order2:vsini" in labels
    packed = [m._pack(None, update_caches=False) for m in models]
    devs, mds = [p[0] for p in packed], [p[1] for p in packed]
    assert not mds[0].has_vsini and mds[1].has_vsini and mds[2].has_vsini
    # the workspace grows by the broadening buffers although segment 0 has none
    lib = devs[0].lib
    plain = _lib.ModelDesc.from_buffer_copy(mds[1])
    plain.has_vsini = 0
    with_rows = [D.to_dev(p[2], devs[0].dev) for p in packed[:2]]
    segs = _segments(devs[:2], with_rows)
    w_union = lib.sf_multi_workspace_bytes_md(segs, 2, D.MultiPlan._desc_array([mds[0], mds[1]]))
    w_plain = lib.sf_multi_workspace_bytes_md(segs, 2, D.MultiPlan._desc_array([mds[0], plain]))
    assert w_union > w_plain > 0
    P = ball(em, B=5, seed=12)
    _, cols = em._layout()
    plans = count_plans(monkeypatch)
    total, info, per_order = em.log_likelihood_batch(P, return_info=True, return_orders=True)
    assert len(plans) == 1 and plans[0].per_order and len(plans[0].calls) == 1
    assert (info == 0).all()
    for i, (o, m) in enumerate(zip(orders, models)):
        oo = oracle_order(o)
        for b in range(len(P)):
            q = oracle_params(m, P[b, cols[i]])
            assert ("vsini" in q) == (i > 0)
            want = O.log_likelihood(oo, q)
            assert close(per_order[i, b], want), (i, b, per_order[i, b], want)
    np.testing.assert_allclose(total, per_order.sum(axis=0), rtol=1e-14)
    for i, m in enumerate(models):
        np.testing.assert_allclose(per_order[i], m.log_likelihood_batch(P[:, cols[i]]), rtol=1e-12)


def test_md_refusal_of_segment_0_names_it():
    """The check of segment 0 runs in the same loop as the others: its refusal names it too."""
    small = synth.make_order(N=6, m=4, seed=3, pad=0.04)
    good_o = TC.make_nf_order(64, seed=5)
    do_small, do_good = device_order(oracle_order(small)), device_order(oracle_order(good_o))
    md_bad = do_small.model_desc(True, True, True, False, 0, 2)
    md_good = do_good.model_desc(True, True, True, False, 0, 2)
    rows = D.to_dev(np.zeros((2, 6 + do_good.P + 2)), do_good.dev)
    segs = _segments([do_small, do_good], [rows, rows])
    lib = do_good.lib
    assert lib.sf_multi_workspace_bytes_md(segs, 2, D.MultiPlan._desc_array([md_bad, md_good])) == 0
    err = lib.sf_last_error().decode()
    assert "segment 0" in err and "16 <= nf <= 65536" in err, err
