"""sf_loglike_multi_grad_batch_md, sf_multi_grad_reduce, EchelleModel's gradient and train, and the one-pass option of
SpectrumModel.log_likelihood_full_gradient_batch: the likelihood of all (order x walker) units and its gradient in every
thawed parameter from ONE factorisation per unit.

Inputs and bounds: tests/echelle_gradient_cases.py (cases A and B: orders of 64 / 130 / 180 and 180 / 64 / 256 pixels with
0 - 3 local kernels, padded to a common npad of 192 and 256; the derived bounds of tests/test_gpu_gradient.py and
tests/test_gpu_mean_gradient.py restated, with the longdouble factor of the reference matrix in the place of the device's).
Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest

from gpu_helpers import oracle_order
from starfish_amd import _device as D
from starfish_amd import _lib, synth

import echelle_gradient_cases as EG

pytestmark = pytest.mark.gpu

_CASES = {}


def case(name):
    """Model, walkers, packed rows and the device results every test of that case shares (made once, never written)."""
    if name not in _CASES:
        orders, models, em, P = EG.build(name)
        labels, cols, requests, sources = em._gradient_layout()
        packed = [m._pack(P[:, cols[i]], update_caches=False) for i, m in enumerate(models)]
        devs, mds, rows = ([p[k] for p in packed] for k in range(3))
        c = dict(orders=orders, models=models, em=em, P=P, labels=labels, cols=cols, requests=requests, sources=sources,
                 devs=devs, mds=mds, rows=rows, npad=EG.CASES[name][3])
        c["out"] = D.loglike_multi_grad(devs, mds, rows, requests)
        c["plist"] = [[EG.oracle_params(m, P[b, cols[i]]) for b in range(len(P))] for i, m in enumerate(models)]
        _CASES[name] = c
    return _CASES[name]


def run_plan(c, requests, sentinel=None):
    plan = D.MultiGradPlan(c["devs"], c["mds"], c["rows"], requests)
    if sentinel is not None:
        plan.grad.fill_(sentinel)
    plan.enqueue()
    return plan, plan.collect()


@pytest.mark.parametrize("name", list(EG.CASES))
def test_no_mu_sits_on_a_kink(name):
    """In mu the likelihood has a kink wherever two pixels of the patch are equidistant from it: the reference's derivative
    is the almost-everywhere one, so every mu keeps 1e-3 pixel from every pixel and every midpoint of two pixels."""
    c = case(name)
    for i, o in enumerate(c["orders"]):
        for b, p in enumerate(c["plist"][i]):
            for off in EG.kink_distances(o["wave"], p):
                print(f"{name} order {i} walker {b}: a mu is {off:.4f} pixel from the nearest kink")
                assert off >= 1e-3


@pytest.mark.parametrize("name", list(EG.CASES))
def test_lnl_info_and_log_scale_have_the_bits_of_the_multi_order_likelihood(name):
    c = case(name)
    assert max(d.npad for d in c["devs"]) == c["npad"] and len({d.npad for d in c["devs"]}) > 1
    ll = D.loglike_multi(c["devs"], c["mds"], c["rows"])
    again = D.loglike_multi_grad(c["devs"], c["mds"], c["rows"], c["requests"])
    for i, (out, ref, rep, md) in enumerate(zip(c["out"], ll, again, c["mds"])):
        assert (ref["info"] == 0).all() and np.isfinite(ref["lnl"]).all()
        for key in ("lnl", "info", "log_scale"):
            np.testing.assert_array_equal(out[key], ref[key], err_msg=f"order {i} {key}")
        assert out["grad"].shape == (3, 8 + 2 + 3 * md.n_local) and np.isfinite(out["grad"]).all()
        for key in ("lnl", "info", "log_scale", "grad"):
            np.testing.assert_array_equal(rep[key], out[key], err_msg=f"order {i} {key} of a repeated call")


@pytest.mark.parametrize("name", list(EG.CASES))
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
            tag = f"{name} order {i} (N = {len(o['wave'])}) walker {b}"
            worst = max(worst, EG.check_mean_slots(tag, oo, p, flux[b], mean, got[:len(mean)]))
            worst = max(worst, EG.check_cov_slots(tag, oo, p, flux[b], c["npad"], got[len(mean):]))
    print(f"{name}: largest err / bound = {worst:.3g}")


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
        for key in ("lnl", "info", "log_scale"):
            np.testing.assert_array_equal(out[i][key], full[i][key])
    raw = plan.grad.cpu().numpy()
    assert plan.stride == 5 and raw.shape == (9, 5)
    assert (raw[0:3, 4:] == -7.0).all() and (raw[6:9] == -7.0).all()  # beyond a row's slots / a segment without a request
    # covariance slots everywhere, mean slots nowhere: one right-hand side per unit
    _, cov = run_plan(c, [([], True)] * 3)
    for i in range(3):
        np.testing.assert_array_equal(cov[i]["grad"], full[i]["grad"][:, 8:])
        np.testing.assert_array_equal(cov[i]["lnl"], full[i]["lnl"])
    # mean slots for the last order alone, a single column for the first
    _, one = run_plan(c, [([cols0[5]], False), ([], False), (c["requests"][2][0], True)])
    np.testing.assert_array_equal(one[0]["grad"][:, 0], full[0]["grad"][:, 5])
    np.testing.assert_array_equal(one[2]["grad"], full[2]["grad"])


def test_a_failed_unit_gets_a_nan_row_and_leaves_every_other_unit_alone():
    c = case("A")
    rows = [r.copy() for r in c["rows"]]
    rows[1][1, 0] = -1.0  # vsini of walker 1 in segment 1
    out = D.loglike_multi_grad(c["devs"], c["mds"], rows, c["requests"])
    assert list(out[1]["info"]) == [0, -2, 0] and np.isneginf(out[1]["lnl"][1]) and np.isnan(out[1]["grad"][1]).all()
    for i in range(3):
        keep = [0, 2] if i == 1 else [0, 1, 2]
        for key in ("lnl", "info", "log_scale", "grad"):
            np.testing.assert_array_equal(out[i][key][keep], c["out"][i][key][keep], err_msg=f"order {i} {key}")


def test_a_walker_outside_the_grid_gets_minus_infinity_and_a_nan_row_through_the_model():
    c = case("B")
    em, P = c["em"], c["P"]
    lnl, grad, info = em.log_likelihood_gradient_batch(P, return_info=True)
    P2 = P.copy()
    P2[1, c["labels"].index("T")] = 9000.0
    lnl2, grad2, info2 = em.log_likelihood_gradient_batch(P2, return_info=True)
    assert list(info) == [0, 0, 0] and list(info2) == [0, -1, 0]
    assert np.isneginf(lnl2[1]) and np.isnan(grad2[1]).all()
    np.testing.assert_array_equal(lnl2[[0, 2]], lnl[[0, 2]])
    np.testing.assert_array_equal(grad2[[0, 2]], grad[[0, 2]])
    np.testing.assert_array_equal(em.last_info, info2)


def test_the_reduce_kernel_against_a_plain_loop():
    """sf_multi_grad_reduce on made-up unit results: a column without a source, columns with one, two and three sources, a
    walker with a failed unit in the first order and one with two failed units (the first code in ascending order counts)."""
    import torch

    lib, dev = _lib.require_gpu(), D.device_of()
    rng = np.random.default_rng(11)
    nseg, W, stride = 3, 70, 7  # (two workgroups' worth of walkers would be 64 columns: here 6 columns, 70 grid planes)
    lnl = rng.standard_normal((nseg, W)) * 1e3
    info = np.zeros((nseg, W), dtype=np.int32)
    info[0, 3], info[1, 40], info[2, 40] = -2, 5, -1
    lnl[0, 3] = lnl[1, 40] = lnl[2, 40] = -np.inf
    grad = rng.standard_normal((nseg, W, stride)) * 10.0 ** rng.integers(-3, 4, size=(nseg, W, stride))
    grad[0, 3] = grad[1, 40] = grad[2, 40] = np.nan
    sources = [[(0, 1), (1, 0), (2, 6)], [], [(2, 0)], [(0, 3), (1, 1)], [(1, 6)], [(0, 0), (2, 2)]]
    col_ptr, col_src = D.column_map_csr(sources)
    want = EG.reduce_restated(lnl, info, list(grad), sources)
    with torch.cuda.device(dev):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        d_lnl, d_info, d_grad, d_ptr, d_src = t(lnl.reshape(-1)), t(info.reshape(-1)), t(grad.reshape(-1, stride)), t(col_ptr), t(col_src)
        outs = []
        for _ in range(2):
            o_lnl, o_grad, o_info = D.empty((W,), dev), torch.full((W, 8), -7.0, dtype=torch.float64, device=dev), D.empty((W,), dev, torch.int32)
            rc = lib.sf_multi_grad_reduce(nseg, W, D.ptr(d_lnl), D.ptr(d_info), D.ptr(d_grad), stride, D.ptr(d_ptr), D.ptr(d_src),
                                          len(sources), D.ptr(o_lnl), D.ptr(o_grad), 8, D.ptr(o_info), D.stream_ptr(dev))
            _lib.check(rc, "sf_multi_grad_reduce")
            outs.append((o_lnl.cpu().numpy(), o_grad.cpu().numpy(), o_info.cpu().numpy()))
        rc = lib.sf_multi_grad_reduce(nseg, W, D.ptr(d_lnl), D.ptr(d_info), D.ptr(d_grad), stride, D.ptr(d_ptr), D.ptr(d_src),
                                      len(sources), D.ptr(o_lnl), D.ptr(o_grad), 5, D.ptr(o_info), D.stream_ptr(dev))
        assert rc == -1 and "out_stride" in lib.sf_last_error().decode()
    (g_lnl, g_grad, g_info), rep = outs
    np.testing.assert_array_equal(g_lnl, want[0])
    np.testing.assert_array_equal(g_grad[:, :6], want[1])
    np.testing.assert_array_equal(g_info, want[2])
    assert (g_grad[:, 6:] == -7.0).all()  # nothing beyond the columns is written
    assert g_info[3] == -2 and g_info[40] == 5 and np.isneginf(g_lnl[[3, 40]]).all() and np.isnan(g_grad[[3, 40], :6]).all()
    assert (g_grad[np.arange(W) != 3][:, 1][np.arange(W - 1) != 39] == 0.0).all()  # the column without a source
    for a, b in zip(outs[0], rep):
        np.testing.assert_array_equal(a, b)


def test_model_gradient_is_the_reduce_of_the_unit_rows_and_leaves_the_state_alone():
    c = case("A")
    em, P, models = c["em"], c["P"], c["models"]
    state = lambda: (tuple(em.get_param_vector()),) + tuple(  # noqa: E731
        (len(m.residuals), m._lnprob, m._log_scale, m._glob_snapshot, str(m._loc_snapshot)) for m in models)
    before = state()
    lnl, grad, info, per_order = em.log_likelihood_gradient_batch(P, return_info=True, return_orders=True)
    unit_lnl = np.stack([o["lnl"] for o in c["out"]])
    unit_info = np.stack([o["info"] for o in c["out"]])
    want = EG.reduce_restated(unit_lnl, unit_info, [o["grad"] for o in c["out"]], c["sources"])
    np.testing.assert_array_equal(lnl, want[0])
    np.testing.assert_array_equal(grad, want[1])
    np.testing.assert_array_equal(info, want[2])
    assert grad.shape == (3, 32) and c["sources"] == EG.expected_sources(em)
    host = D.reduce_orders_host(unit_lnl, unit_info, [o["grad"] for o in c["out"]], c["sources"])  # (orders on several devices)
    for a, b in zip(host, want):
        np.testing.assert_array_equal(a, b)
    total, _, orders_ll = em.log_likelihood_batch(P, return_info=True, return_orders=True)
    np.testing.assert_allclose(lnl, total, rtol=1e-14)
    np.testing.assert_array_equal(per_order, orders_ll)
    # frozen labels: the walkers sit at the model's own value there, and the remaining columns keep their bits
    frozen = ["vz", "order1:cheb:1"]
    labels = list(c["labels"])
    P2 = P.copy()
    for key in frozen:
        P2[:, labels.index(key)] = em.get_param_vector()[labels.index(key)]
    _, g_all = em.log_likelihood_gradient_batch(P2)
    em.freeze(frozen)
    try:
        keep = [j for j, key in enumerate(labels) if key not in frozen]
        assert list(em.labels) == [labels[j] for j in keep]
        _, g_kept = em.log_likelihood_gradient_batch(P2[:, keep])
    finally:
        em.thaw(frozen)
    np.testing.assert_array_equal(g_kept, g_all[:, keep])
    # the scalar form at the current state
    l1, g1 = em.log_likelihood_gradient()
    la, ga = em.log_likelihood_gradient_batch(em.get_param_vector()[None, :])
    assert l1 == la[0] and tuple(g1) == tuple(labels)
    np.testing.assert_array_equal(list(g1.values()), ga[0])
    assert state() == before


def test_one_pass_full_gradient_of_a_single_order():
    o = synth.make_order(N=180, m=4, seed=5)
    model = synth.build_model(o)
    P = synth.walker_ball(o, B=3, seed=3)
    labels = model.labels
    lnl, grad, info = model.log_likelihood_full_gradient_batch(P, return_info=True, one_pass=True)
    assert grad.shape == (3, len(labels)) and list(info) == [0, 0, 0]
    dev, md, rows = model._pack(P, update_caches=False)
    np.testing.assert_array_equal(lnl, D.loglike_multi([dev], [md], [rows])[0]["lnl"])
    oo = oracle_order(o)
    flux = dev.apply(md, rows, "Cinv", want_flux=True)["flux"]
    mean, cov = model.mean_gradient_labels, model.gradient_labels
    assert dev.npad == 192 and [labels.index(k) for k in cov] == sorted(labels.index(k) for k in cov)
    for b, vec in enumerate(P):
        p = synth.vector_to_oracle_params(vec)
        EG.check_mean_slots(f"one pass walker {b}", oo, p, flux[b], mean, grad[b, [labels.index(k) for k in mean]])
        EG.check_cov_slots(f"one pass walker {b}", oo, p, flux[b], dev.npad, grad[b, [labels.index(k) for k in cov]])
    # the default: today's two calls and their bits
    l2, g2 = model.log_likelihood_full_gradient_batch(P)
    lm, gm = model.log_likelihood_mean_gradient_batch(P)
    lc, gc = model.log_likelihood_gradient_batch(P)
    np.testing.assert_array_equal(g2[:, [labels.index(k) for k in mean]], gm)
    np.testing.assert_array_equal(g2[:, [labels.index(k) for k in cov]], gc)
    np.testing.assert_array_equal(l2, lc)


def test_train_does_not_decrease_the_likelihood_and_leaves_the_model_at_the_solution():
    _, _, em, P = EG.build("A")
    em.set_param_vector(P[0])
    start = em.log_likelihood_gradient_batch(P[:1])[0][0]
    soln = em.train(options=dict(maxiter=3))
    print(f"EchelleModel.train(maxiter=3): {soln.message}; nit {soln.nit}, nfev {soln.nfev}; lnL {start!r} -> {-soln.fun!r}")
    assert soln.x.shape == (len(em.labels),) and -soln.fun >= start
    np.testing.assert_array_equal(em.get_param_vector(), soln.x)


def _raw_call(c, mds, requests, stride):
    """The C entry points themselves: (return code, message, workspace query, lnl as left on the device)."""
    import torch

    devs = c["devs"]
    lib, dev = devs[0].lib, devs[0].dev
    with torch.cuda.device(dev):
        Pd = [D.to_dev(r, dev) for r in c["rows"]]
        segs = (_lib.Segment * len(devs))()
        for k, (d, r) in enumerate(zip(devs, Pd)):
            segs[k] = _lib.Segment(d.ctx, D.ptr(r).value, int(r.shape[0]), 0)
        models = D.MultiPlan._desc_array(list(mds))
        keep = [(C.c_int32 * max(len(cols), 1))(*cols) for cols, _ in requests]
        reqs = (_lib.GradRequest * len(devs))()
        for k, ((cols, cov), arr) in enumerate(zip(requests, keep)):
            reqs[k] = _lib.GradRequest(arr, len(cols), int(cov))
        U = sum(int(r.shape[0]) for r in Pd)
        query = lib.sf_multi_grad_workspace_bytes_md(segs, len(devs), models, reqs, stride)
        ok_reqs, ok_keep = _requests(c["requests"])  # (the call that is not refused sizes the workspace)
        ok = lib.sf_multi_grad_workspace_bytes_md(segs, len(devs), D.MultiPlan._desc_array(list(c["mds"])), ok_reqs, 19)
        ws = D.workspace(ok, dev)
        lnl = torch.full((U,), -7.0, dtype=torch.float64, device=dev)
        info, grad = D.empty((U,), dev, torch.int32), D.empty((U, 32), dev)
        rc = lib.sf_loglike_multi_grad_batch_md(segs, len(devs), models, reqs, D.ptr(lnl), None, D.ptr(info), D.ptr(grad), stride,
                                                D.ptr(ws), ws.numel(), D.stream_ptr(dev))
        msg = lib.sf_last_error().decode()
        torch.cuda.synchronize(dev)
        return rc, msg, query, lnl.cpu().numpy()


def _requests(requests):
    keep = [(C.c_int32 * max(len(cols), 1))(*cols) for cols, _ in requests]
    reqs = (_lib.GradRequest * len(requests))()
    for k, ((cols, cov), arr) in enumerate(zip(requests, keep)):
        reqs[k] = _lib.GradRequest(arr, len(cols), int(cov))
    return reqs, keep


def _desc(md, **change):
    other = _lib.ModelDesc()
    for name, _ in md._fields_:
        setattr(other, name, change.get(name, getattr(md, name)))
    return other


def test_requests_the_device_does_not_differentiate_are_refused_before_anything_is_enqueued():
    c = case("A")
    mds, req = c["mds"], c["requests"]
    rc, msg, query, lnl = _raw_call(c, mds, req, 19)
    assert rc == 0 and query > 0 and np.isfinite(lnl).all(), msg
    bad = {
        "no log_scale": ([mds[0], _desc(mds[1], has_log_scale=0), mds[2]], req, 19, r"segment 1: .*log_scale"),
        "want_cov without kernels": ([_desc(mds[0], has_global=0), mds[1], mds[2]], req, 19, r"segment 0: nothing to differentiate"),
        "a repeated column": (mds, [req[0], req[1], (req[2][0][:3] + [req[2][0][1]], True)], 19, r"segment 2: column 0 is listed twice"),
        "a covariance column as a mean slot": (mds, [req[0], ([4], False), req[2]], 19, r"segment 1: column 4 is not"),
        "grad_stride too small": (mds, req, 18, r"segment 2: grad_stride=18 < 19 slots"),
        "no request at all": (mds, [([], False)] * 3, 19, r"nothing to differentiate"),
    }
    for what, (models, requests, stride, pattern) in bad.items():
        rc, msg, query, lnl = _raw_call(c, models, requests, stride)
        assert rc == -1 and query == 0, (what, rc, query, msg)
        assert "sf_loglike_multi_grad_batch_md" in msg and __import__("re").search(pattern, msg), (what, msg)
        assert (lnl == -7.0).all(), what  # nothing ran
