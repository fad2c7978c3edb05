"""The selected inversion on the band (sf_band_selinv_batch) and the covariance gradient on the band + Woodbury solver
(sf_loglike_banded_grad_batch through DeviceOrder.loglike_grad(solver=...), DeviceOrder.loglike_banded_grad and the
SpectrumModel methods).

Stand-alone call: strictly diagonally dominant band matrices (tests/band_selinv_reference.band_spd, 3 per shape) at shapes that
cover a single block, a window wider than the matrix, partial last blocks, the sliding window and the widest one.  The
reference is the block recurrence in np.longdouble (tests/band_selinv_reference.py; its agreement with a dense inverse is
tests/test_banded_cov_gradient_host.py's), the bound per entry selinv_bound, evaluated from the reference's factor alone:
(|X| dA |X|)_ij + gamma_2n (E + E^T)_ij + gamma_{n+1} (|Xl|^T |Xl|)_ij, dA = 1e-13 |A| + gamma_{W+17} |L||L|^T.

Model: the cases of tests/test_gpu_gradient.py, built as it builds them, plus m = 17 and a narrow global kernel (the window
slides over most of the matrix).  Every walker's host half-width bound lies inside the window, every walker comes back with
info == 0 and every mu keeps 1e-3 pixel from every kink, which the tests assert: no case may skip, fall back or sit on a kink.
Every slot is held to the dense test's bound (its docstring, items 1 - 4), evaluated from the np.longdouble reference alone: L
is the longdouble Cholesky factor of the oracle's matrix rounded to float64, X its inverse.  That bound is derived for a
dense inverse, not for C^-1 = Sigma - Vs Vs^T: the dense call goes through the same check (soft) as the yardstick, and both
fractions are printed per case."""
import numpy as np
import pytest

from oracle import sf_oracle as O
from starfish_amd import _device as D
from starfish_amd import _lib, synth

import band_selinv_reference as SR
import cov_derivatives as CD
from gpu_helpers import device_order, oracle_order, pack_rows
from test_gpu_banded_gradient import run_band_solve
from test_gpu_gradient import cholesky_longdouble, gamma, inverse_longdouble, oracle_params
from test_gpu_mean_gradient import MEAN, columns
from test_gpu_model import close_lnl

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
SENTINEL = 7.0


# ------------------------------------------------------------------------------------------ the stand-alone call
def run_band_selinv(bands, ldb, n, w):
    import torch

    lib = _lib.require_gpu()
    dev = D.device_of()
    batch, ldo = bands.shape[0], w + 2
    d_band = D.to_dev(bands, dev)
    out = D.to_dev(np.full((batch, n + 1, ldo), SENTINEL), dev)  # (a row and a column the call must leave alone)
    logdet = D.empty((batch,), dev)
    info = D.empty((batch,), dev, torch.int32)
    need = lib.sf_band_selinv_workspace_bytes(n, w, batch)
    assert need > 0
    ws = D.empty((need,), dev, torch.uint8)
    rc = lib.sf_band_selinv_batch(D.ptr(d_band), n, w, ldb, n * ldb, batch, D.ptr(out), ldo, (n + 1) * ldo, D.ptr(logdet), D.ptr(info),
                                  D.ptr(ws), need, D.stream_ptr(dev))
    _lib.check(rc, "sf_band_selinv_batch")
    return dict(out=out.cpu().numpy(), logdet=logdet.cpu().numpy(), info=info.cpu().numpy(), band=d_band.cpu().numpy())


@pytest.mark.parametrize("n,w", [(16, 0), (40, 60), (64, 63), (100, 5), (257, 16), (257, 37), (333, 80), (300, 128), (500, 144),
                                 (2048, 31)])
def test_band_selinv_within_the_entrywise_bound_of_the_longdouble_recurrence(n, w):
    rng = np.random.default_rng(100 * n + w)
    mats, bands = [], []
    for _ in range(3):
        A, band, ldb = SR.band_spd(rng, n, w)
        mats.append(A)
        bands.append(band)
    bands = np.stack(bands)
    got = run_band_selinv(bands, ldb, n, w)
    assert (got["info"] == 0).all()
    np.testing.assert_array_equal(got["band"], bands)  # d_band is not modified
    mask = SR.on_band(n, w)
    worst = 0.0
    for b in range(3):
        ref = SR.selected_inverse(mats[b].astype(LD), w, LD)
        bound = SR.selinv_bound(mats[b], w, ref["L"])
        sig = got["out"][b, :n, : w + 1]
        err = np.abs(sig - ref["band"].astype(np.float64))
        ratio = float((err[mask] / bound[mask]).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (b, ratio)
        # nothing but the band's own entries is written: not d > i, not the column behind the band, not the row behind the matrix
        assert (sig[~mask] == SENTINEL).all() and (got["out"][b, :, w + 1] == SENTINEL).all() and (got["out"][b, n] == SENTINEL).all()
    print(f"n={n} w={w}: largest err / bound = {worst:.3g}")
    solve = run_band_solve(bands, ldb, n, w, rng.standard_normal((3, 1, n)))
    np.testing.assert_array_equal(got["logdet"], solve["logdet"])
    again = run_band_selinv(bands, ldb, n, w)
    for key in ("out", "logdet", "info"):
        np.testing.assert_array_equal(again[key], got[key], err_msg=key)


def test_band_selinv_not_positive_definite_gets_nan_and_leaves_its_neighbours_alone():
    rng = np.random.default_rng(3)
    n, w = 200, 7
    _, band, ldb = SR.band_spd(rng, n, w)
    bad = band.copy()
    bad[77, 0] = -1.0  # pivot 78 (1-based) becomes negative
    _, other, _ = SR.band_spd(rng, n, w)
    mask = SR.on_band(n, w)
    out = run_band_selinv(np.stack([band, bad, other]), ldb, n, w)
    assert out["info"].tolist() == [0, 78, 0]
    assert np.isnan(out["out"][1, :n, : w + 1][mask]).all() and np.isfinite(out["out"][[0, 2]]).all()
    good = run_band_selinv(np.stack([band, band, other]), ldb, n, w)
    np.testing.assert_array_equal(out["out"][[0, 2]], good["out"][[0, 2]])
    np.testing.assert_array_equal(out["logdet"][[0, 2]], good["logdet"][[0, 2]])


# ------------------------------------------------------------------------------------------ the model
CASES = ["N180", "N256", "N330", "N180-two-local", "N180-global", "N180-m17", "N330-narrow"]
_CASES = {}


def case(name):
    """Order, DeviceOrder, rows and the device results every test of that case shares (made once, never written)."""
    if name not in _CASES:
        N, m = int(name[1:4]), 17 if name.endswith("m17") else 4
        o = synth.make_order(N=N, m=m, seed=5)
        oo = oracle_order(o)
        do = device_order(oo)
        P = synth.walker_ball(o, B=3, seed=3)
        plist = [oracle_params(o, name, p) for p in P]
        if name.endswith("narrow"):
            for p in plist:
                p["global_cov"] = (p["global_cov"][0], float(np.log(2.0)))
        md, rows = pack_rows(do, plist)
        c = dict(N=N, m=m, o=o, oo=oo, do=do, P=P, plist=plist, md=md, rows=rows)
        c["hw"] = do.halfwidth_bound(md, rows)
        c["out"] = do.loglike_grad(md, rows, want_flux=True, solver="banded")
        c["dense"] = do.loglike_grad(md, rows, want_flux=True)
        _CASES[name] = c
    return _CASES[name]


@pytest.mark.parametrize("name", CASES)
def test_every_case_runs_on_the_band_solver_away_from_the_kinks(name):
    c = case(name)
    do = c["do"]
    print(name, "half-width bounds", c["hw"], "window", do.banded_window_halfwidth())
    assert c["hw"].max() <= do.banded_window_halfwidth() <= 144
    if "global_cov" in c["plist"][0] and "local_cov" in c["plist"][0] and not name.endswith("narrow"):
        assert 115 <= c["hw"].min() and c["hw"].max() <= 119
    assert c["hw"].max() <= 119
    assert (c["out"]["info"] == 0).all() and np.isfinite(c["out"]["grad"]).all()
    w = c["o"]["wave"]
    mids = 0.5 * (w[:, None] + w[None, :])
    for p in c["plist"]:
        for mu, _, _ in p.get("local_cov", []):
            k = int(np.clip(np.searchsorted(w, mu), 1, len(w) - 1))
            assert np.abs(mids - mu).min() / (w[k] - w[k - 1]) >= 1e-3


@pytest.mark.parametrize("name", CASES)
def test_shape_lnl_and_info(name):
    c = case(name)
    do, md, rows, out, dense = c["do"], c["md"], c["rows"], c["out"], c["dense"]
    assert out["grad"].shape == dense["grad"].shape and out["lnl"].shape == (3,) and out["flux"].shape == (3, c["N"])
    mean = do.loglike_mean_grad(md, rows, [2], solver="banded")  # the same sweep on the same right-hand sides
    np.testing.assert_array_equal(out["lnl"], mean["lnl"])
    np.testing.assert_array_equal(out["info"], mean["info"])
    assert (dense["info"] == 0).all()
    for b in range(3):
        assert close_lnl(out["lnl"][b], dense["lnl"][b])
    np.testing.assert_allclose(out["flux"], dense["flux"], rtol=0, atol=1e-12 * np.abs(dense["flux"]).max())


def reference(c, b, flux):
    """The longdouble reference of walker b for the residual flux - data and the dense test's bound per slot, from the
    reference alone."""
    key = ("ref", b, flux.tobytes())
    if key not in c:
        oo, N, npad, p = c["oo"], c["N"], c["do"].npad, c["plist"][b]
        wave = c["o"]["wave"]
        C64 = O.forward_model(oo, p)[1] + 1e-10 * np.eye(N)
        Lref = cholesky_longdouble(C64.astype(LD))
        Xr = inverse_longdouble(Lref)
        Cinv = Xr.T @ Xr
        r64 = flux - oo.flux
        alpha = Cinv @ r64.astype(LD)
        A = np.outer(alpha, alpha) - Cinv
        aL, aX = np.abs(Lref).astype(np.float64), np.abs(Xr).astype(np.float64)  # (the reference factor rounded to float64)
        aCi, aal, aA = np.abs(Cinv).astype(np.float64), np.abs(alpha).astype(np.float64), np.abs(A).astype(np.float64)
        dC = 1e-13 * np.abs(C64) + gamma(npad + 1) * (aL @ aL.T)
        solve = (1e-13 + N * gamma(3 * N + 1)) * (np.abs(C64).sum(axis=1).max() * aal.max() + np.abs(r64).max())
        d_alpha = aCi @ (dC @ aal) + aCi.sum(axis=1) * solve
        E = aX.T @ (aX @ (aL @ aX))
        dG = aCi @ dC @ aCi + gamma(2 * npad) * (E + E.T) + gamma(npad + 1) * (aX.T @ aX)
        first = np.outer(d_alpha, aal) + np.outer(aal, d_alpha) + dG
        second = 3 * U * (np.outer(aal, aal) + aCi)
        A64 = np.outer(*(np.linalg.solve(C64, r64),) * 2) - np.linalg.inv(C64)
        slots = []
        for (label, d), (_, dbar), (_, d64) in zip(CD.slot_derivatives(wave, p, dtype=LD), CD.slot_derivatives(wave, p, absolute=True),
                                                   CD.slot_derivatives(wave, p)):
            size = 0.5 * np.sum(aA * dbar)
            k = int(np.count_nonzero(dbar))
            bound = 0.5 * np.sum(first * dbar) + 0.5 * np.sum(second * dbar) + 1e-13 * size + gamma(k) * size
            slots.append((label, float(0.5 * np.sum(A * d)), float(0.5 * np.sum(A64 * d64)), float(size), float(bound)))
        c[key] = slots
    return c[key]


def check_slots(name, c, out, hard):
    """Every slot of out["grad"] against the longdouble reference: the dense test's bound and its wrong-weight guard.  Prints
    every figure; asserts both when ``hard``.  Returns the largest err / bound."""
    worst = 0.0
    for b in range(3):
        slots = reference(c, b, out["flux"][b])
        assert len(slots) == out["grad"].shape[1]
        for s, (label, ref, ref64, size, bound) in enumerate(slots):
            got = out["grad"][b, s]
            err = abs(got - ref)
            worst = max(worst, err / bound)
            print(f"{name} walker {b} {label}: {got!r}, err / bound = {err / bound:.3g} (bound {bound:.3g}), "
                  f"|got - float64 reference| / (1/2 sum |A| Dbar) = {abs(got - ref64) / size:.3g}")
            if hard:
                assert err <= bound, (name, b, label, got, ref, err, bound)
                assert abs(got - ref64) <= 1e-6 * size, (name, b, label, got, ref64, size)
    return worst


@pytest.mark.parametrize("name", CASES)
def test_every_slot_within_the_dense_tests_bound_of_the_longdouble_reference(name):
    c = case(name)
    banded = check_slots(name + " banded", c, c["out"], hard=True)
    dense = check_slots(name + " dense", c, c["dense"], hard=False)
    print(f"{name}: largest err / bound: banded {banded:.3g}, dense {dense:.3g}")


@pytest.mark.parametrize("name", CASES)
def test_repeated_and_chunked_calls_give_the_same_bits(name):
    c = case(name)
    do, md, rows = c["do"], c["md"], c["rows"]
    kw = dict(want_flux=True, solver="banded")
    for other in (do.loglike_grad(md, rows, **kw), do.loglike_grad(md, rows, max_chunk=1, **kw)):
        for key in ("lnl", "grad", "info", "flux"):
            np.testing.assert_array_equal(other[key], c["out"][key], err_msg=key)
    # the dense call keeps its bits beside the new one
    again = do.loglike_grad(md, rows, want_flux=True)
    for key in ("lnl", "grad", "info", "flux"):
        np.testing.assert_array_equal(again[key], c["dense"][key], err_msg=key)


@pytest.mark.parametrize("name", ["N256", "N180-two-local", "N180-m17"])
def test_combined_call_has_the_bits_of_the_two_separate_calls(name):
    c = case(name)
    do, md, rows = c["do"], c["md"], c["rows"]
    slots = columns(do, md, MEAN)
    mean = do.loglike_mean_grad(md, rows, slots, solver="banded")
    both = do.loglike_banded_grad(md, rows, slots, True)
    ncov = c["out"]["grad"].shape[1]
    assert both["grad"].shape == (3, len(slots) + ncov)
    np.testing.assert_array_equal(both["grad"][:, : len(slots)], mean["grad"])
    np.testing.assert_array_equal(both["grad"][:, len(slots):], c["out"]["grad"])
    np.testing.assert_array_equal(both["lnl"], mean["lnl"])
    np.testing.assert_array_equal(both["info"], mean["info"])
    pick = slots[::-2]
    sub = do.loglike_banded_grad(md, rows, pick, True, max_chunk=1)
    np.testing.assert_array_equal(sub["grad"][:, len(pick):], c["out"]["grad"])
    np.testing.assert_array_equal(sub["grad"][:, : len(pick)], mean["grad"][:, ::-2])
    only_mean = do.loglike_banded_grad(md, rows, slots, False)
    np.testing.assert_array_equal(only_mean["grad"], mean["grad"])
    with pytest.raises(ValueError, match="nothing to differentiate"):
        do.loglike_banded_grad(md, rows, [], False)


def test_failed_walkers_get_nan_rows_and_leave_the_others_alone():
    c = case("N256")
    do, md = c["do"], c["md"]
    rows = c["rows"].copy()
    rows[1, 0] = -1.0
    rows[2, 6] = 1e5
    out = do.loglike_grad(md, rows, want_flux=True, solver="banded")
    dense = do.loglike_grad(md, rows, want_flux=True)
    np.testing.assert_array_equal(out["info"], dense["info"])
    assert list(out["info"]) == [0, -2, -1] and np.isneginf(out["lnl"][1:]).all() and np.isneginf(dense["lnl"][1:]).all()
    assert np.isnan(out["grad"][1:]).all() and np.isnan(dense["grad"][1:]).all()
    for key in ("grad", "lnl", "flux"):
        np.testing.assert_array_equal(out[key][0], c["out"][key][0])


def test_a_walker_wider_than_the_window_is_flagged_and_auto_sends_it_to_the_dense_call():
    c = case("N256")
    do = c["do"]
    plist = [dict(p) for p in c["plist"]]
    plist[1]["global_cov"] = (plist[1]["global_cov"][0], float(np.log(14.0)))
    md, rows = pack_rows(do, plist)
    hw = do.halfwidth_bound(md, rows)
    print("half-width bounds", hw)
    assert hw[1] > do.banded_window_halfwidth() and hw[0] <= do.banded_window_halfwidth() and hw[2] <= do.banded_window_halfwidth()
    out = do.loglike_grad(md, rows, solver="banded")
    assert out["info"].tolist() == [0, D.INFO_BANDWIDTH, 0] and out["lnl"][1] == -np.inf and np.isnan(out["grad"][1]).all()
    for key in ("grad", "lnl"):
        np.testing.assert_array_equal(out[key][[0, 2]], c["out"][key][[0, 2]])
    auto = do.loglike_grad(md, rows, solver="auto")
    dense = do.loglike_grad(md, rows)
    assert (auto["info"] == 0).all()
    for key in ("grad", "lnl"):
        np.testing.assert_array_equal(auto[key][1], dense[key][1])
        np.testing.assert_array_equal(auto[key][[0, 2]], c["out"][key][[0, 2]])
    both = do.loglike_banded_grad(md, rows, [2], True, solver="auto")
    np.testing.assert_array_equal(both["grad"][1, 1:], dense["grad"][1])
    np.testing.assert_array_equal(both["grad"][1, :1], do.loglike_mean_grad(md, rows[1:2], [2])["grad"][0])
    np.testing.assert_array_equal(both["grad"][[0, 2], 1:], c["out"]["grad"][[0, 2]])
    # the C-ABI: a half-width below a walker's support flags it; one beyond the window is refused, naming the dense call
    ncov, none = c["out"]["grad"].shape[1], (_lib.C.c_int * 1)()  # (no mean slots: the array is not read)
    with pytest.raises(_lib.StarfishAMDError, match="sf_loglike_grad_batch"):
        do._run_grad("loglike_banded_grad_batch", md, rows, (do.banded_window_halfwidth() + 1, none, 0, 1), ncov, lambda units: 1 << 20,
                     False, None)
    low = do._run_grad("loglike_banded_grad_batch", c["md"], c["rows"], (16, none, 0, 1), ncov,
                       lambda units: do.loglike_banded_grad_workspace_bytes(c["md"], units, 16, 0, True), False, None)
    assert (low["info"] == D.INFO_BANDWIDTH).all() and np.isneginf(low["lnl"]).all() and np.isnan(low["grad"]).all()


def test_model_methods_take_the_solver_and_default_to_the_dense_bits():
    c = case("N256")
    model = synth.build_model(c["o"])
    dev, md, rows = model._pack(c["P"], update_caches=False)
    raw = dev.loglike_grad(md, rows, solver="auto")
    dense = dev.loglike_grad(md, rows)
    lnl, g = model.log_likelihood_gradient_batch(c["P"], solver="auto")
    np.testing.assert_array_equal(lnl, raw["lnl"])
    np.testing.assert_array_equal(g, raw["grad"])
    assert not np.array_equal(g, dense["grad"])  # (another inverse: agreement to rounding, not bit for bit)
    for built_with in ("dense", "auto"):
        other = synth.build_model(c["o"], solver=built_with)
        lnl0, g0 = other.log_likelihood_gradient_batch(c["P"])
        np.testing.assert_array_equal(g0, dense["grad"])
        np.testing.assert_array_equal(lnl0, dense["lnl"])
    model.set_param_vector(c["P"][0])
    l1, g1 = model.log_likelihood_gradient(solver="banded")
    assert l1 == raw["lnl"][0] and tuple(g1) == model.gradient_labels
    np.testing.assert_array_equal(np.array(list(g1.values())), raw["grad"][0])
    l0, g0 = model.log_likelihood_gradient()
    assert l0 == dense["lnl"][0]
    np.testing.assert_array_equal(np.array(list(g0.values())), dense["grad"][0])
    # the full gradient: one combined device call where both solvers are the band solver's; what it was without the new argument
    labels = model.labels
    slots = columns(dev, md, MEAN)
    both = dev.loglike_banded_grad(md, rows, slots, True, solver="auto")
    lnl, full = model.log_likelihood_full_gradient_batch(c["P"], solver="auto", covariance_solver="auto")
    np.testing.assert_array_equal(lnl, both["lnl"])
    np.testing.assert_array_equal(full[:, [labels.index(k) for k in MEAN]], both["grad"][:, : len(slots)])
    np.testing.assert_array_equal(full[:, [labels.index(k) for k in model.gradient_labels]], both["grad"][:, len(slots):])
    lnl, full = model.log_likelihood_full_gradient_batch(c["P"], solver="auto")
    np.testing.assert_array_equal(full[:, [labels.index(k) for k in model.gradient_labels]], dense["grad"])
    np.testing.assert_array_equal(lnl, dense["lnl"])
    lnl, full = model.log_likelihood_full_gradient_batch(c["P"], covariance_solver="banded")  # (two calls: dense mean columns)
    np.testing.assert_array_equal(full[:, [labels.index(k) for k in model.gradient_labels]], raw["grad"])
    np.testing.assert_array_equal(full[:, [labels.index(k) for k in MEAN]], dev.loglike_mean_grad(md, rows, slots)["grad"])


def test_training_on_the_banded_gradient_does_not_decrease_the_likelihood():
    c = case("N180")
    model = synth.build_model(c["o"])
    for key in ("global_cov:log_amp", "global_cov:log_ls", "local_cov:0:log_amp", "local_cov:0:log_sigma"):
        model[key] = model[key] + 0.5
    displaced = model.get_param_vector().copy()
    start = model.log_likelihood()
    soln = model.train_covariance(gradient_solver="auto", options=dict(maxiter=3))
    print(f"train_covariance(gradient_solver='auto', maxiter=3): {soln.message}; nit {soln.nit}, nfev {soln.nfev}; "
          f"lnL {start!r} -> {-soln.fun!r}")
    assert np.isfinite(soln.fun) and model.log_likelihood() >= start
    model.set_param_vector(displaced)
    soln = model.train(gradient=True, gradient_solver="auto", covariance_solver="auto", options=dict(maxiter=3))
    print(f"train(gradient=True, gradient_solver='auto', covariance_solver='auto', maxiter=3): {soln.message}; nit {soln.nit}, "
          f"nfev {soln.nfev}; lnL {start!r} -> {-soln.fun!r}")
    assert np.isfinite(soln.fun) and model.log_likelihood() >= start
