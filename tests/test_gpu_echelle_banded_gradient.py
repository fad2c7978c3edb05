"""sf_loglike_banded_multi_grad_batch_md, BandedMultiGradPlan and EchelleModel's ``solver=``: the likelihood of all
(order x walker) units and its gradient in every thawed parameter on the band + Woodbury solver, one launch sequence per device.

Inputs: tests/echelle_banded_cases.py (cases A, B of tests/echelle_gradient_cases.py: half-widths wider than the 64-pixel
orders, orders of different length in one frame; case C: bounds 36 - 38 beside 119 - 126, the longest order not the widest;
C-wide: one unit beyond any window).  Bounds: EG.check_mean_slots / EG.check_cov_slots, the derived bounds of the dense tests
(from the np.longdouble reference and the oracle's matrix; derived for a Cholesky solve, so not tight for the band solver: the
largest err / bound per case is printed).  Status -2 is reached as tests/test_gpu_echelle_gradient.py reaches it (a negative
vsini), -1 by a walker off the grid.  Run with -m gpu."""
import numpy as np
import pytest

from gpu_helpers import oracle_order
from starfish_amd import _device as D
from test_gpu_model import close_lnl

import echelle_banded_cases as EB
import echelle_gradient_cases as EG

pytestmark = pytest.mark.gpu

_CASES = {}
KEYS = ("lnl", "info", "log_scale", "grad")


def case(name):
    """Model, walkers, packed rows and the device results every test of that case shares (made once, never written)."""
    if name not in _CASES:
        orders, models, em, P = EB.build(name)
        labels, cols, requests, sources = em._gradient_layout(solver="banded")
        packed = [m._pack(P[:, cols[i]], update_caches=False) for i, m in enumerate(models)]
        devs, mds, rows = ([p[k] for p in packed] for k in range(3))
        c = dict(orders=orders, models=models, em=em, P=P, labels=labels, cols=cols, requests=requests, sources=sources,
                 devs=devs, mds=mds, rows=rows, npad=max(d.npad for d in devs))
        c["plan"] = D.loglike_banded_multi_grad(devs, mds, rows, requests, sync=False)
        c["out"] = c["plan"].collect()
        c["plist"] = [[EG.oracle_params(m, P[b, cols[i]]) for b in range(len(P))] for i, m in enumerate(models)]
        _CASES[name] = c
    return _CASES[name]


def same(a, b, keys=KEYS, rows=None, msg=""):
    for key in keys:
        x, y = (a[key], b[key]) if rows is None else (a[key][rows], b[key][rows])
        np.testing.assert_array_equal(x, y, err_msg=f"{msg} {key}")


@pytest.mark.parametrize("name", EB.CASES)
def test_every_unit_slot_within_its_bound_of_the_longdouble_reference(name):
    c = case(name)
    worst = 0.0
    for i, (o, m, dev, md, rows) in enumerate(zip(c["orders"], c["models"], c["devs"], c["mds"], c["rows"])):
        oo = oracle_order(o)
        flux = dev.apply(md, rows, "Cinv", want_flux=True)["flux"]  # (the transform chain's own: the residual of the bound)
        mean = m.mean_gradient_labels
        assert len(mean) == len(c["requests"][i][0]) == 8
        for b, p in enumerate(c["plist"][i]):
            got = c["out"][i]["grad"][b]
            assert got.shape == (8 + 2 + 3 * md.n_local,)
            tag = f"{name} order {i} (N = {len(o['wave'])}) walker {b}"
            worst = max(worst, EG.check_mean_slots(tag, oo, p, flux[b], mean, got[:len(mean)]))
            worst = max(worst, EG.check_cov_slots(tag, oo, p, flux[b], c["npad"], got[len(mean):]))
    print(f"{name}: largest err / bound = {worst:.3g}")


@pytest.mark.parametrize("name", EB.CASES)
def test_lnl_info_and_log_scale_per_unit_and_a_repeated_call(name):
    c = case(name)
    plan = c["plan"]
    assert plan.complete and plan.rerouted == 0 and plan.halfwidth == max(int(b.max()) for b in plan.bounds)
    for i, (b, (lo, hi)) in enumerate(zip(plan.bounds, EB.BOUNDS[name])):
        assert (b >= lo).all() and (b <= hi).all() and c["devs"][i].banded_window_halfwidth() == EB.WINDOW
    if name != "C":
        assert plan.halfwidth > min(d.n for d in c["devs"])  # a half-width larger than an order
    dense = D.loglike_multi(c["devs"], c["mds"], c["rows"])
    again = D.loglike_banded_multi_grad(c["devs"], c["mds"], c["rows"], c["requests"])
    for i, (out, ref, rep) in enumerate(zip(c["out"], dense, again)):
        assert (out["info"] == 0).all() and (ref["info"] == 0).all(), (i, out["info"])
        for b in range(3):
            print(f"{name} order {i} walker {b}: lnl {out['lnl'][b]!r}, dense {ref['lnl'][b]!r}")
            assert close_lnl(out["lnl"][b], ref["lnl"][b]), (i, b, out["lnl"][b], ref["lnl"][b])
        np.testing.assert_array_equal(out["log_scale"], ref["log_scale"])
        assert np.isfinite(out["grad"]).all()
        same(rep, out, msg=f"order {i} of a repeated call")


@pytest.mark.parametrize("name,caps", [("A", (4, 2, 5, 7)), ("C", (4,))])
def test_a_plan_cut_into_several_calls_gives_the_bits_of_one_call(name, caps):
    """A cap of 4 units splits the 9 units of A between its orders and leaves a last piece of one order; 2, 5 and 7 cut elsewhere."""
    c = case(name)
    for cap in caps:
        plan = D.BandedMultiGradPlan(c["devs"], c["mds"], c["rows"], c["requests"], max_units=cap)
        assert len(plan.plan.calls) == -(-9 // cap) and plan.halfwidth == c["plan"].halfwidth
        if cap == 4:  # 3 + 1 | 2 + 2 | 1: cut inside orders 1 and 2, a last piece of order 2 alone
            assert [[i for i, _, _ in piece] for piece in plan.plan.pieces] == [[0, 1], [1, 2], [2]]
        plan.enqueue()
        for i, (out, full) in enumerate(zip(plan.collect(), c["out"])):
            same(out, full, msg=f"max_units={cap} order {i}")


def run_plan(c, requests, sentinel=None):
    plan = D.BandedMultiGradPlan(c["devs"], c["mds"], c["rows"], requests)
    if sentinel is not None:
        plan.plan.grad.fill_(sentinel)
    plan.enqueue()
    return plan, plan.collect()


def test_subsets_of_the_request_give_the_bits_of_the_full_call_and_touch_nothing_else():
    c = case("A")
    full = c["out"]
    cols0 = c["requests"][0][0]
    pick = list(range(len(cols0)))[::-2]
    # order 0: every second mean column in reverse order and no covariance slots; order 1: covariance slots alone;
    # order 2: nothing
    plan, out = run_plan(c, [([cols0[j] for j in pick], False), ([], True), ([], False)], sentinel=-7.0)
    np.testing.assert_array_equal(out[0]["grad"], full[0]["grad"][:, pick])
    np.testing.assert_array_equal(out[1]["grad"], full[1]["grad"][:, 8:])
    assert out[2]["grad"].shape == (3, 0)
    for i in range(3):
        same(out[i], full[i], keys=("lnl", "info", "log_scale"))
    raw = plan.plan.grad.cpu().numpy()
    assert plan.plan.stride == 5 and raw.shape == (9, 5)
    assert (raw[0:3, 4:] == -7.0).all() and (raw[6:9] == -7.0).all()  # beyond a row's slots / a segment without a request
    # covariance slots everywhere, mean slots nowhere
    _, cov = run_plan(c, [([], True)] * 3)
    for i in range(3):
        np.testing.assert_array_equal(cov[i]["grad"], full[i]["grad"][:, 8:])
        np.testing.assert_array_equal(cov[i]["lnl"], full[i]["lnl"])
    # mean slots for the last order alone, a single column for the first
    _, one = run_plan(c, [([cols0[5]], False), ([], False), (c["requests"][2][0], True)])
    np.testing.assert_array_equal(one[0]["grad"][:, 0], full[0]["grad"][:, 5])
    np.testing.assert_array_equal(one[2]["grad"], full[2]["grad"])


def test_order_sum_on_the_device_equals_the_host_rule_and_the_model_returns_it():
    c = case("A")
    em, P = c["em"], c["P"]
    unit_lnl, unit_info = np.stack([o["lnl"] for o in c["out"]]), np.stack([o["info"] for o in c["out"]])
    grads = [o["grad"] for o in c["out"]]
    got = c["plan"].reduce(c["sources"])
    host = D.reduce_orders_host(unit_lnl, unit_info, grads, c["sources"])
    for a, b in zip(got, host):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(got, EG.reduce_restated(unit_lnl, unit_info, grads, c["sources"])):
        np.testing.assert_array_equal(a, b)
    lnl, grad, info, per_order = em.log_likelihood_gradient_batch(P, return_info=True, return_orders=True, solver="banded")
    np.testing.assert_array_equal(lnl, got[0])
    np.testing.assert_array_equal(grad, got[1])
    np.testing.assert_array_equal(info, got[2])
    np.testing.assert_array_equal(per_order, unit_lnl)
    assert grad.shape == (3, 32) and list(info) == [0, 0, 0]
    l1, g1 = em.log_likelihood_gradient(solver="banded")
    la, ga = em.log_likelihood_gradient_batch(em.get_param_vector()[None, :], solver="banded")
    assert l1 == la[0]
    np.testing.assert_array_equal(list(g1.values()), ga[0])


def test_defaults_keep_the_bits_of_the_dense_call():
    c = case("B")
    em, P, models = c["em"], c["P"], c["models"]
    today = em.log_likelihood_gradient_batch(P, return_info=True)
    for solver in (None, "dense"):
        for a, b in zip(em.log_likelihood_gradient_batch(P, return_info=True, solver=solver), today):
            np.testing.assert_array_equal(a, b)
    models[1].solver = "auto"  # "dense" selects the dense call whatever the orders' own solver is
    try:
        for a, b in zip(em.log_likelihood_gradient_batch(P, return_info=True, solver="dense"), today):
            np.testing.assert_array_equal(a, b)
        with pytest.raises(ValueError, match="order 1: .*dense"):
            em.log_likelihood_gradient_batch(P)
    finally:
        models[1].solver = "dense"


def test_failed_units_get_a_nan_row_and_leave_every_other_unit_alone():
    c = case("A")
    rows = [r.copy() for r in c["rows"]]
    rows[1][1, 0] = -1.0  # vsini of walker 1 in segment 1: status -2
    out = D.loglike_banded_multi_grad(c["devs"], c["mds"], rows, c["requests"])
    assert list(out[1]["info"]) == [0, -2, 0] and np.isneginf(out[1]["lnl"][1]) and np.isnan(out[1]["grad"][1]).all()
    for i in range(3):
        same(out[i], c["out"][i], rows=[0, 2] if i == 1 else [0, 1, 2], msg=f"order {i}")
    # through the model: a walker off the grid (-1) and one with a negative vsini (-2)
    em, P, labels = c["em"], c["P"], list(c["labels"])
    lnl, grad, info = em.log_likelihood_gradient_batch(P, return_info=True, solver="banded")
    P2 = P.copy()
    P2[1, labels.index("T")] = 9000.0
    P2[2, labels.index("vsini")] = -1.0
    lnl2, grad2, info2 = em.log_likelihood_gradient_batch(P2, return_info=True, solver="banded")
    assert list(info) == [0, 0, 0] and list(info2) == [0, -1, -2]
    assert np.isneginf(lnl2[1:]).all() and np.isnan(grad2[1:]).all()
    np.testing.assert_array_equal(lnl2[0], lnl[0])
    np.testing.assert_array_equal(grad2[0], grad[0])
    np.testing.assert_array_equal(em.last_info, info2)
    # a unit off the grid in one order alone: every other unit keeps its bits
    rows = [r.copy() for r in c["rows"]]
    rows[2][0, 6] = 9000.0  # T of walker 0 in segment 2 alone: status -1
    out = D.loglike_banded_multi_grad(c["devs"], c["mds"], rows, c["requests"])
    assert list(out[2]["info"]) == [-1, 0, 0] and np.isneginf(out[2]["lnl"][0]) and np.isnan(out[2]["grad"][0]).all()
    for i in range(3):
        same(out[i], c["out"][i], rows=[1, 2] if i == 2 else [0, 1, 2], msg=f"order {i}")


def test_a_unit_beyond_the_window_is_refused_under_banded_and_dense_under_auto():
    c = case("C")
    orders, models, em, P = EB.build("C-wide")
    labels, cols, requests, sources = em._gradient_layout(solver="auto")
    packed = [m._pack(P[:, cols[i]], update_caches=False) for i, m in enumerate(models)]
    devs, mds, rows = ([p[k] for p in packed] for k in range(3))
    # "banded": the unit is refused, its walker is -inf with a NaN row after the order sum
    plan = D.loglike_banded_multi_grad(devs, mds, rows, requests, solver="banded", sync=False)
    out = plan.collect()
    assert [list(f) for f in plan.fits] == [[True] * 3, [True, False, True], [True] * 3] and not plan.complete
    assert plan.halfwidth == c["plan"].halfwidth  # (the group's largest bound is that of case C: same frame, same bits)
    assert out[1]["info"][1] == D.INFO_BANDWIDTH and np.isneginf(out[1]["lnl"][1]) and np.isnan(out[1]["grad"][1]).all()
    for i in range(3):
        same(out[i], c["out"][i], rows=[0, 2] if i == 1 else [0, 1, 2], msg=f"banded order {i}")
    lnl, grad, info = plan.reduce(sources)
    want = c["plan"].reduce(c["sources"])
    assert list(info) == [0, D.INFO_BANDWIDTH, 0] and np.isneginf(lnl[1]) and np.isnan(grad[1]).all()
    np.testing.assert_array_equal(lnl[[0, 2]], want[0][[0, 2]])
    np.testing.assert_array_equal(grad[[0, 2]], want[1][[0, 2]])
    got = em.log_likelihood_gradient_batch(P, return_info=True, solver="banded")
    for a, b in zip(got, (lnl, grad, info)):
        np.testing.assert_array_equal(a, b)
    # "auto": that unit has the bits of the dense call on its row, every other unit those of case C
    plan = D.loglike_banded_multi_grad(devs, mds, rows, requests, solver="auto", sync=False)
    out = plan.collect()
    assert plan.rerouted == 1 and all((o["info"] == 0).all() for o in out)
    dense = D.loglike_multi_grad([devs[1]], [mds[1]], [rows[1][1:2]], [requests[1]])[0]
    for key in KEYS:
        np.testing.assert_array_equal(out[1][key][1], dense[key][0], err_msg=key)
    for i in range(3):
        same(out[i], c["out"][i], rows=[0, 2] if i == 1 else [0, 1, 2], msg=f"auto order {i}")
    lnl, grad, info = em.log_likelihood_gradient_batch(P, return_info=True, solver="auto")
    host = D.reduce_orders_host(np.stack([o["lnl"] for o in out]), np.stack([o["info"] for o in out]), [o["grad"] for o in out], sources)
    for a, b in zip((lnl, grad, info), host):
        np.testing.assert_array_equal(a, b)
    assert list(info) == [0, 0, 0] and np.isfinite(grad).all()
    np.testing.assert_array_equal(lnl[[0, 2]], want[0][[0, 2]])
    np.testing.assert_array_equal(grad[[0, 2]], want[1][[0, 2]])


def test_train_on_the_band_solver_does_not_decrease_the_likelihood_and_leaves_the_model_at_the_solution():
    _, _, em, P = EB.build("A")
    em.set_param_vector(P[0])
    start = em.log_likelihood_gradient_batch(P[:1], solver="auto")[0][0]
    soln = em.train(gradient_solver="auto", options=dict(maxiter=3))
    print(f"EchelleModel.train(gradient_solver='auto', maxiter=3): {soln.message}; nit {soln.nit}, nfev {soln.nfev}; "
          f"lnL {start!r} -> {-soln.fun!r}")
    assert soln.x.shape == (len(em.labels),) and -soln.fun >= start
    np.testing.assert_array_equal(em.get_param_vector(), soln.x)
