"""The full banded solve (sf_band_solve_batch) and the mean-flux gradient on the band + Woodbury solver
(sf_loglike_banded_mean_grad_batch through DeviceOrder.loglike_mean_grad(solver=...) and the SpectrumModel methods).

Stand-alone solve: the matrices of tests/test_gpu_banded.py (random_band_spd, batch 3) at shapes that cover a single block, a
window wider than the matrix, partial last blocks, one to three blocks of right-hand sides and the three window limits; per
right-hand side the residual bound of tests/test_gpu_apply_factor.py, |A x - b|_inf <= fac (|A|_inf |x|_inf + |b|_inf) with
fac = 1e-13 + n gamma_{3n+1}.

Model: the orders and walkers of tests/test_gpu_mean_gradient.py (make_order(seed=5), walker_ball(B=3, seed=3)); their host
half-width bounds are 115 .. 119 pixels at every N, inside the window for m = 4 (144) and m = 17 (128), which the tests assert:
no case may skip or fall back.  Every slot is held to the dense test's reference-only bound (tests/banded_derivatives.py,
check_slots), which is derived for a Cholesky solve, not for Woodbury: the dense call sits far inside it and serves as the
yardstick; the largest fraction of the bound is printed for both calls on the same case."""
import numpy as np
import pytest

from starfish_amd import _device as D
from starfish_amd import _lib, synth

import banded_derivatives as BD
from gpu_helpers import device_order, oracle_order, pack_rows
from test_gpu_banded import random_band_spd, run_band_forms
from test_gpu_mean_gradient import MEAN, columns
from test_gpu_model import close_lnl

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------ the stand-alone solve
def run_band_solve(bands, ldb, n, w, rhs, want_gram=True):
    import torch

    lib = _lib.require_gpu()
    dev = D.device_of()
    batch, nrhs = rhs.shape[0], rhs.shape[1]
    d_band = D.to_dev(bands, dev)
    d_rhs = D.to_dev(rhs, dev)
    x = D.empty((batch, nrhs, n), dev)
    logdet = D.empty((batch,), dev)
    gram = D.empty((batch, nrhs, nrhs), dev) if want_gram else None
    info = D.empty((batch,), dev, torch.int32)
    need = lib.sf_band_solve_workspace_bytes(n, w, batch, nrhs)
    assert need > 0
    ws = D.empty((need,), dev, torch.uint8)
    rc = lib.sf_band_solve_batch(D.ptr(d_band), n, w, ldb, n * ldb, batch, D.ptr(d_rhs), nrhs, n, nrhs * n, D.ptr(x), n, nrhs * n,
                                 D.ptr(logdet), D.ptr(gram) if want_gram else None, D.ptr(info), D.ptr(ws), need, D.stream_ptr(dev))
    _lib.check(rc, "sf_band_solve_batch")
    out = dict(x=x.cpu().numpy(), logdet=logdet.cpu().numpy(), info=info.cpu().numpy(), band=d_band.cpu().numpy())
    if want_gram:
        out["gram"] = gram.cpu().numpy()
    return out


def band_batch(rng, n, w, batch=3):
    mats, bands = [], []
    w_eff = min(w, n - 1)
    for _ in range(batch):
        A, band, ldb = random_band_spd(rng, n, w_eff)
        if w_eff < w:  # storage wider than the matrix: extra diagonals are zero
            ldb2 = w + 1 + (w + 1) % 2
            b2 = np.zeros((n, ldb2))
            b2[:, : band.shape[1]] = band
            band, ldb = b2, ldb2
        mats.append(A)
        bands.append(band)
    return mats, np.stack(bands), ldb


@pytest.mark.parametrize("n,w,nrhs", [(16, 0, 1), (40, 60, 2), (64, 63, 3), (100, 5, 9), (257, 16, 9), (257, 37, 20), (333, 80, 33),
                                       (300, 128, 17), (500, 144, 9), (2048, 31, 9)])
def test_band_solve_vs_numpy(n, w, nrhs):
    rng = np.random.default_rng(100 * n + w)
    mats, bands, ldb = band_batch(rng, n, w)
    rhs = rng.standard_normal((3, nrhs, n))
    out = run_band_solve(bands, ldb, n, w, rhs)
    assert (out["info"] == 0).all()
    np.testing.assert_array_equal(out["band"], bands)  # d_band is not modified
    fac = BD.solve_factor(n)
    worst = 0.0
    for b in range(3):
        A = mats[b]
        anorm = np.abs(A).sum(axis=1).max()
        for r in range(nrhs):
            x = out["x"][b, r]
            res = np.abs(A @ x - rhs[b, r]).max()
            bound = fac * (anorm * np.abs(x).max() + np.abs(rhs[b, r]).max())
            worst = max(worst, res / bound)
            assert res <= bound, (b, r, res, bound)
        sign, want_ld = np.linalg.slogdet(A)
        assert sign > 0 and abs(out["logdet"][b] - want_ld) <= 1e-12 * max(1.0, abs(want_ld))
    print(f"n={n} w={w} nrhs={nrhs}: largest residual / bound = {worst:.3g}")
    _, gram, _ = run_band_forms(bands, ldb, n, w, rhs)
    np.testing.assert_allclose(out["gram"], gram, rtol=1e-11)
    again = run_band_solve(bands, ldb, n, w, rhs, want_gram=False)  # (no Gram matrix asked for: the workspace's)
    for key in ("x", "logdet", "info"):
        np.testing.assert_array_equal(again[key], out[key], err_msg=key)


def test_band_solve_not_positive_definite_gets_nan_and_leaves_its_neighbours_alone():
    rng = np.random.default_rng(3)
    n, w = 200, 7
    A, band, ldb = random_band_spd(rng, n, w)
    bad = band.copy()
    bad[77, 0] = -1.0  # pivot 78 (1-based) becomes negative
    _, other, _ = random_band_spd(rng, n, w)
    rhs = rng.standard_normal((3, 2, n))
    out = run_band_solve(np.stack([band, bad, other]), ldb, n, w, rhs)
    assert out["info"].tolist() == [0, 78, 0]
    assert np.isnan(out["x"][1]).all() and np.isfinite(out["x"][[0, 2]]).all()
    good = run_band_solve(np.stack([band, band, other]), ldb, n, w, rhs)
    np.testing.assert_array_equal(out["x"][[0, 2]], good["x"][[0, 2]])
    np.testing.assert_array_equal(out["logdet"][[0, 2]], good["logdet"][[0, 2]])


# ------------------------------------------------------------------------------------------ the model
CASES = ["N180", "N256", "N330", "N180-Av", "N180-m17", "N330-narrow"]
_CASES = {}


def case(name):
    """Order, DeviceOrder, rows and the device results every test of that case shares (made once, never written)."""
    if name not in _CASES:
        N, m = int(name[1:4]), 17 if name.endswith("m17") else 4
        o = synth.make_order(N=N, m=m, seed=5)
        oo = oracle_order(o)
        do = device_order(oo)
        P = synth.walker_ball(o, B=3, seed=3)
        plist = [synth.vector_to_oracle_params(p) for p in P]
        labels = MEAN
        if name.endswith("Av"):
            for p in plist:
                del p["vz"], p["vsini"]
                p["Av"] = 0.3
            labels = ("log_scale", "cheb:1", "cheb:2", "T", "logg", "Z", "Av")
        if name.endswith("narrow"):  # the window slides over most of the matrix
            for p in plist:
                p["global_cov"] = (p["global_cov"][0], float(np.log(2.0)))
        md, rows = pack_rows(do, plist)
        c = dict(N=N, m=m, o=o, oo=oo, do=do, P=P, plist=plist, md=md, rows=rows, labels=labels, slots=columns(do, md, labels))
        c["hw"] = do.halfwidth_bound(md, rows)
        assert c["hw"].max() <= do.banded_window_halfwidth(), (c["hw"], do.banded_window_halfwidth())
        c["out"] = do.loglike_mean_grad(md, rows, c["slots"], want_flux=True, solver="banded")
        c["dense"] = do.loglike_mean_grad(md, rows, c["slots"], want_flux=True)
        _CASES[name] = c
    return _CASES[name]


@pytest.mark.parametrize("name", CASES)
def test_lnl_info_and_flux_agree_with_loglike(name):
    c = case(name)
    do, md, rows, out = c["do"], c["md"], c["rows"], c["out"]
    print(name, "half-width bounds", c["hw"], "window", do.banded_window_halfwidth())
    assert out["grad"].shape == (3, len(c["labels"])) and out["lnl"].shape == (3,) and out["flux"].shape == (3, c["N"])
    assert (out["info"] == 0).all() and np.isfinite(out["grad"]).all()
    dense = do.loglike(md, rows)
    band = do.loglike(md, rows, solver="banded")
    assert (dense["info"] == 0).all() and (band["info"] == 0).all()
    for b in range(3):
        assert close_lnl(out["lnl"][b], dense["lnl"][b]) and close_lnl(out["lnl"][b], band["lnl"][b])
    np.testing.assert_allclose(out["flux"], c["dense"]["flux"], rtol=0, atol=1e-12 * np.abs(c["dense"]["flux"]).max())


@pytest.mark.parametrize("name", CASES)
def test_repeated_chunked_and_subset_calls_give_the_same_bits(name):
    c = case(name)
    do, md, rows, slots = c["do"], c["md"], c["rows"], c["slots"]
    kw = dict(want_flux=True, solver="banded")
    for other in (do.loglike_mean_grad(md, rows, slots, **kw), do.loglike_mean_grad(md, rows, slots, max_chunk=1, **kw)):
        for key in ("lnl", "grad", "info", "flux"):
            np.testing.assert_array_equal(other[key], c["out"][key], err_msg=key)
    pick = list(range(len(slots)))[::-2]
    sub = do.loglike_mean_grad(md, rows, [slots[j] for j in pick], solver="banded")
    np.testing.assert_array_equal(sub["grad"], c["out"]["grad"][:, pick])
    np.testing.assert_array_equal(sub["lnl"], c["out"]["lnl"])
    for j in (0, len(slots) - 1, c["labels"].index("T")):
        np.testing.assert_array_equal(do.loglike_mean_grad(md, rows, [slots[j]], solver="banded")["grad"][:, 0], c["out"]["grad"][:, j])
    # the dense call keeps its bits beside the new one
    np.testing.assert_array_equal(do.loglike_mean_grad(md, rows, slots)["grad"], c["dense"]["grad"])


@pytest.mark.parametrize("name", CASES)
def test_every_slot_within_the_dense_tests_bound_of_the_longdouble_reference(name):
    c = case(name)
    banded = BD.check_slots(name + " banded", c["oo"], c["plist"], c["labels"], c["out"], hard=True)
    dense = BD.check_slots(name + " dense", c["oo"], c["plist"], c["labels"], c["dense"], hard=False)
    print(f"{name}: largest err / bound: banded {banded:.3g}, dense {dense:.3g}")


def test_failed_walkers_get_nan_rows_and_leave_the_others_alone():
    c = case("N256")
    do, md, slots = c["do"], c["md"], c["slots"]
    rows = c["rows"].copy()
    rows[1, 0] = -1.0
    rows[2, 6] = 1e5
    out = do.loglike_mean_grad(md, rows, slots, want_flux=True, solver="banded")
    dense = do.loglike_mean_grad(md, rows, slots, want_flux=True)
    np.testing.assert_array_equal(out["info"], dense["info"])
    assert list(out["info"]) == [0, -2, -1] and np.isneginf(out["lnl"][1:]).all()
    assert np.isnan(out["grad"][1:]).all()
    for key in ("grad", "lnl", "flux"):
        np.testing.assert_array_equal(out[key][0], c["out"][key][0])


def test_a_walker_wider_than_the_window_is_flagged_and_auto_sends_it_to_the_dense_call():
    c = case("N256")
    do, slots = c["do"], c["slots"]
    plist = [dict(p) for p in c["plist"]]
    plist[1]["global_cov"] = (plist[1]["global_cov"][0], float(np.log(14.0)))
    md, rows = pack_rows(do, plist)
    hw = do.halfwidth_bound(md, rows)
    print("half-width bounds", hw)
    assert hw[1] > do.banded_window_halfwidth() and hw[0] <= do.banded_window_halfwidth() and hw[2] <= do.banded_window_halfwidth()
    out = do.loglike_mean_grad(md, rows, slots, solver="banded")
    assert out["info"].tolist() == [0, D.INFO_BANDWIDTH, 0] and out["lnl"][1] == -np.inf and np.isnan(out["grad"][1]).all()
    for key in ("grad", "lnl"):
        np.testing.assert_array_equal(out[key][[0, 2]], c["out"][key][[0, 2]])
    auto = do.loglike_mean_grad(md, rows, slots, solver="auto")
    dense = do.loglike_mean_grad(md, rows, slots)
    assert (auto["info"] == 0).all()
    for key in ("grad", "lnl"):
        np.testing.assert_array_equal(auto[key][1], dense[key][1])
        np.testing.assert_array_equal(auto[key][[0, 2]], c["out"][key][[0, 2]])
    # the C-ABI: a half-width below a walker's support flags it; one beyond the window is refused, naming the dense call
    with pytest.raises(_lib.StarfishAMDError, match="sf_loglike_mean_grad_batch"):
        do._run_grad("loglike_banded_mean_grad_batch", md, rows, (do.banded_window_halfwidth() + 1, (_lib.C.c_int * 1)(2), 1), 1,
                     lambda units: 1 << 20, False, None)
    low = do._run_grad("loglike_banded_mean_grad_batch", c["md"], c["rows"], (16, (_lib.C.c_int * 1)(2), 1), 1,
                       lambda units: do.loglike_banded_mean_grad_workspace_bytes(c["md"], units, 16, 1), False, None)
    assert (low["info"] == D.INFO_BANDWIDTH).all() and np.isneginf(low["lnl"]).all() and np.isnan(low["grad"]).all()


def test_model_methods_take_the_solver_and_default_to_the_dense_bits():
    c = case("N256")
    model = synth.build_model(c["o"])
    dev, md, rows = model._pack(c["P"], update_caches=False)
    raw = dev.loglike_mean_grad(md, rows, columns(dev, md, MEAN), solver="auto")
    lnl, g = model.log_likelihood_mean_gradient_batch(c["P"], solver="auto")
    np.testing.assert_array_equal(lnl, raw["lnl"])
    np.testing.assert_array_equal(g, raw["grad"])
    dense = dev.loglike_mean_grad(md, rows, columns(dev, md, MEAN))
    assert not np.array_equal(g, dense["grad"])  # (another solve: agreement to rounding, not bit for bit)
    for built_with in ("dense", "auto"):
        other = synth.build_model(c["o"], solver=built_with)
        lnl0, g0 = other.log_likelihood_mean_gradient_batch(c["P"])
        np.testing.assert_array_equal(g0, dense["grad"])
        np.testing.assert_array_equal(lnl0, dense["lnl"])
    model.set_param_vector(c["P"][0])
    l1, g1 = model.log_likelihood_mean_gradient(solver="banded")
    assert l1 == raw["lnl"][0] and tuple(g1) == MEAN
    np.testing.assert_array_equal(np.array([g1[k] for k in MEAN]), raw["grad"][0])
    labels = model.labels
    lnl, full = model.log_likelihood_full_gradient_batch(c["P"], solver="auto")
    np.testing.assert_array_equal(full[:, [labels.index(k) for k in MEAN]], g)
    lc, gc = model.log_likelihood_gradient_batch(c["P"])
    np.testing.assert_array_equal(full[:, [labels.index(k) for k in model.gradient_labels]], gc)
    np.testing.assert_array_equal(lnl, lc)


def test_train_with_the_banded_gradient_does_not_decrease_the_likelihood():
    c = case("N256")
    model = synth.build_model(c["o"])
    model.set_param_vector(c["P"][0])
    start = model.log_likelihood()
    soln = model.train(gradient=True, gradient_solver="auto", options=dict(maxiter=3))
    print(f"train(gradient=True, gradient_solver='auto', maxiter=3): {soln.message}; nit {soln.nit}, nfev {soln.nfev}; "
          f"lnL {start!r} -> {-soln.fun!r}")
    assert np.isfinite(soln.fun) and model.log_likelihood() >= start
