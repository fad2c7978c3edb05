"""sf_loglike_mean_grad_batch through DeviceOrder.loglike_mean_grad and the SpectrumModel methods: the gradient of the
likelihood in the mean-flux parameters (vsini, vz, log_scale, Av, cheb:k, the emulator's grid parameters).

Orders, all with three walkers of walker_ball(seed=3) on make_order(seed=5): N = 180 (npad 192: the factorisation's shifted
frame, a partial last 64-row block, one 256-pixel block), 256 and 330 (two pixel blocks, the second partial) with m = 4; N = 180
with Av and without vz / vsini (the context's static spline coefficients); N = 180 with m = 17 (1 + m = 18 right-hand sides:
two groups of the solve, the second partial); N = 256 with a walker of vsini = -1 and one with T outside the grid.

Every slot is held to a bound against the np.longdouble contraction of tests/mean_derivatives.py, which takes the oracle's
matrix plus jitter, the device's own flux for the residual and float64 rows and tangents.  u = 2^-53, gamma_k = k u / (1 - k u):
  (1) the solve: |dalpha| <= |C^-1| e fac (|C|_inf |alpha|_inf + |r|_inf), fac = 1e-13 + N gamma_{3N+1}, and the same for every
      column of V = C^-1 X^T with its right-hand side (the residual bound of tests/test_gpu_apply_factor.py), carried to first
      order through the four terms: for a row tangent (df, dX)
          sum_i |dalpha|_i (|df|_i + sum_k |dX|_ki |za|_k) + sum_ik |dX|_ki |alpha|_i (|S^-1| |X| |dalpha|)_k + sum_ik |dX|_ki (|dV| |S^-1|)_ik,
      for a grid tangent (dmu, dS), with da = |X| |dalpha|, dza = |S^-1| da, dG = |S^-1| |X| |dV| |S^-1|:
          |dmu|^T da + |za|^T |dS| dza + 1/2 sum |dS| o dG;
  (2) the transform contract, 1e-10 max|row|, on the tangents: 1e-10 (max|df| sum_i |alpha|_i + max|dX| sum_ik |omega|_ik);
  (3) gamma_k S_q for the sums, k their number of terms (N (1 + 2 m) for a row tangent, m + 2 m^2 for a grid tangent), and
      3 u S_q for the three roundings per product;
  (4) what is not derived -- the transform contract on the rows themselves, which enter C, and the rounding of the grid
      tangents, whose Sigma_w' = -(z'^T z + z^T z') cancels -- is covered as follows: 8 x the difference between the float64 and
      the longdouble contraction (both references) for another order of summation, plus 1e-10 S_q for the rows.
S_q is the sum with every term replaced by its absolute value (vz, vsini and T are 1e-3 beside terms of order 1e2).  A
wrong-weight guard on top, the hard assertion: every slot agrees with the float64 helper to 1e-6 S_q (a dropped product-rule
half or a wrong sign is off by order 1e-1)."""
import numpy as np
import pytest

from starfish_amd import _lib, synth

import mean_derivatives as MD
from gpu_helpers import device_order, oracle_order, pack_rows

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
MEAN = tuple(k for k in synth.LABELS if not k.startswith(("global_cov", "local_cov")))
CASES = ["N180", "N256", "N330", "N180-Av", "N180-m17"]


def gamma(k):
    return k * U / (1 - k * U)


def columns(do, md, labels):
    P = do.P
    col = {"vsini": 0, "vz": 1, "log_scale": 2, "T": 6, "logg": 7, "Z": 8}
    col.update({f"cheb:{k + 1}": 6 + P + k for k in range(md.n_cheb)})
    col["Av"] = 6 + P + md.n_cheb + 3 * md.n_local
    return [col[k] for k in labels]


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
        md, rows = pack_rows(do, plist)
        c = dict(N=N, m=m, o=o, oo=oo, do=do, P=P, plist=plist, md=md, rows=rows, labels=labels, slots=columns(do, md, labels))
        c["out"] = do.loglike_mean_grad(md, rows, c["slots"], want_flux=True)
        _CASES[name] = c
    return _CASES[name]


@pytest.mark.parametrize("name", CASES)
def test_lnl_info_and_flux_have_the_bits_of_loglike_and_apply(name):
    c = case(name)
    do, md, rows, out = c["do"], c["md"], c["rows"], c["out"]
    assert out["grad"].shape == (3, len(c["labels"])) and out["lnl"].shape == (3,) and out["flux"].shape == (3, c["N"])
    ll = do.loglike(md, rows)
    assert (ll["info"] == 0).all()
    np.testing.assert_array_equal(out["lnl"], ll["lnl"])
    np.testing.assert_array_equal(out["info"], ll["info"])
    np.testing.assert_array_equal(out["flux"], do.apply(md, rows, "Cinv", want_flux=True)["flux"])
    assert np.isfinite(out["grad"]).all()


@pytest.mark.parametrize("name", CASES)
def test_repeated_chunked_and_subset_calls_give_the_same_bits(name):
    c = case(name)
    do, md, rows, slots = c["do"], c["md"], c["rows"], c["slots"]
    for other in (do.loglike_mean_grad(md, rows, slots, want_flux=True), do.loglike_mean_grad(md, rows, slots, want_flux=True, max_chunk=1)):
        for key in ("lnl", "grad", "info", "flux"):
            np.testing.assert_array_equal(other[key], c["out"][key], err_msg=key)
    # subsets: every second column in reverse order, and each kind alone
    pick = list(range(len(slots)))[::-2]
    sub = do.loglike_mean_grad(md, rows, [slots[j] for j in pick])
    np.testing.assert_array_equal(sub["grad"], c["out"]["grad"][:, pick])
    np.testing.assert_array_equal(sub["lnl"], c["out"]["lnl"])
    for j in (0, len(slots) - 1, c["labels"].index("T")):
        np.testing.assert_array_equal(do.loglike_mean_grad(md, rows, [slots[j]])["grad"][:, 0], c["out"]["grad"][:, j])


@pytest.mark.parametrize("name", CASES)
def test_every_slot_within_its_bound_of_the_longdouble_reference(name):
    c = case(name)
    oo, N, m, labels = c["oo"], c["N"], c["m"], c["labels"]
    fac = 1e-13 + N * gamma(3 * N + 1)
    worst = 0.0
    for b, p in enumerate(c["plist"]):
        flux = c["out"]["flux"][b]
        ref64 = MD.gradient(oo, p, labels)
        q = {}
        refld = MD.gradient(oo, p, labels, dtype=LD, flux=flux, pieces=q)
        own64 = MD.gradient(oo, p, labels, flux=flux)
        ab = lambda v: np.abs(v).astype(np.float64)  # noqa: E731
        aCi, aX, aSi, aal, aza = np.abs(np.linalg.inv(q["C"])), ab(q["X"]), ab(q["Sinv"]), ab(q["alpha"]), ab(q["za"])
        cnorm, rowsum = np.abs(q["C"]).sum(axis=1).max(), aCi.sum(axis=1)
        d_alpha = rowsum * fac * (cnorm * aal.max() + ab(q["r"]).max())
        d_V = np.stack([rowsum * fac * (cnorm * ab(q["V"][:, k]).max() + aX[k].max()) for k in range(m)], axis=1)
        omega = np.outer(aal, aza) + ab(q["W"])  # (N, m)
        for j, label in enumerate(labels):
            got = c["out"]["grad"][b, j]
            kind, d0, d1 = q["tan"][label]
            d0, d1 = np.abs(d0), np.abs(d1)
            sq = float(refld[label][1])
            if kind == "rows":
                solve = (d_alpha @ (d0 + d1.T @ aza) + np.sum(d1.T * np.outer(aal, aSi @ (aX @ d_alpha)))
                         + np.sum(d1.T * (d_V @ aSi)))
                contract = 1e-10 * (d0.max() * aal.sum() + d1.max() * omega.sum())
                k = N * (1 + 2 * m)
            else:
                da = aX @ d_alpha
                solve = d0 @ da + aza @ (d1 @ (aSi @ da)) + 0.5 * np.sum(d1 * (aSi @ (aX @ d_V) @ aSi))
                contract = 0.0
                k = m + 2 * m * m
            other_order = 8 * abs(float(own64[label][0] - refld[label][0]))
            bound = solve + contract + (gamma(k) + 3 * U) * sq + other_order + 1e-10 * sq
            err = abs(float(got - refld[label][0]))
            guard = abs(got - ref64[label][0]) / float(ref64[label][1])
            worst = max(worst, err / bound)
            print(f"{name} walker {b} {label}: {got!r}, err / bound = {err / bound:.3g} (bound {bound:.3g}: solve {solve:.3g}, "
                  f"contract {contract:.3g}, 8 x |float64 - longdouble| {other_order:.3g}), S_q {sq:.3g}, "
                  f"|got - float64 helper| / S_q = {guard:.3g}")
            assert guard <= 1e-6, (name, b, label, got, ref64[label])
            assert err <= bound, (name, b, label, got, float(refld[label][0]), err, bound)
    print(f"{name}: largest err / bound = {worst:.3g}")


def test_failed_walkers_get_nan_rows_and_leave_the_others_alone():
    c = case("N256")
    do, md, slots = c["do"], c["md"], c["slots"]
    rows = c["rows"].copy()
    rows[1, 0] = -1.0
    rows[2, 6] = 1e5
    out = do.loglike_mean_grad(md, rows, slots, want_flux=True)
    ll = do.loglike(md, rows)
    np.testing.assert_array_equal(out["info"], ll["info"])
    np.testing.assert_array_equal(out["lnl"], ll["lnl"])
    assert list(out["info"]) == [0, -2, -1] and np.isneginf(out["lnl"][1:]).all()
    assert np.isnan(out["grad"][1:]).all()
    np.testing.assert_array_equal(out["grad"][0], c["out"]["grad"][0])
    np.testing.assert_array_equal(out["lnl"][0], c["out"]["lnl"][0])
    np.testing.assert_array_equal(out["flux"][0], c["out"]["flux"][0])


def test_columns_and_models_that_are_not_differentiated_are_refused_with_a_message():
    c = case("N180")
    do, md, rows = c["do"], c["md"], c["rows"]
    P = do.P
    bad = {
        "norm": [3], "global log_amp": [4], "global log_ls": [5], "a local-kernel column": [6 + P + 2], "past the row": [6 + P + 2 + 3],
        "negative": [-1], "twice": [1, 2, 1], "none": [], "too many": list(range(3)) * 6,
    }
    for what, slots in bad.items():
        with pytest.raises(_lib.StarfishAMDError, match="sf_loglike_mean_grad_batch"):
            do.loglike_mean_grad(md, rows, slots)
    h = (_lib.C.c_int * 2)(1, 2)
    ws = do._reserve(do.loglike_mean_grad_workspace_bytes(md, 3, 2))
    from starfish_amd._device import ptr, to_dev
    Pd = to_dev(rows, do.dev)
    g = to_dev(np.zeros((3, 2)), do.dev)
    rc = do.lib.sf_loglike_mean_grad_batch(do.ctx, _lib.C.byref(md), 3, ptr(Pd), h, 2, ptr(g), ptr(g), 1, None, None, ptr(ws), ws.numel(), None)
    assert rc == -1 and "grad_stride" in do.lib.sf_last_error().decode()
    for change, word in ((dict(has_log_scale=0), "log_scale"), (dict(use_sigma_w=1), "use_sigma_w")):
        other = do.model_desc(md.has_vsini, md.has_vz, md.has_log_scale, md.has_global, md.n_local, md.n_cheb)
        for key, v in change.items():
            setattr(other, key, v)
        with pytest.raises(_lib.StarfishAMDError, match=word):
            do.loglike_mean_grad(other, rows, [2])
    sizes = np.array([do.loglike_mean_grad_workspace_bytes(md, B, 8) for B in (1, 2, 3, 64)])
    assert (np.diff(sizes) > 0).all() and do.loglike_mean_grad_workspace_bytes(md, 0, 8) == 0
    assert do.loglike_mean_grad_workspace_bytes(md, 3, 0) == 0 and do.loglike_mean_grad_workspace_bytes(md, 3, 17) == 0
    assert do.loglike_mean_grad_workspace_bytes(md, 3, 8) > do.apply_workspace_bytes(md, 3, 5)


def test_model_methods_return_the_columns_of_the_thawed_labels():
    c = case("N256")
    model = synth.build_model(c["o"])
    l0 = model.log_likelihood()
    before = (len(model.residuals), model._lnprob, model._log_scale, model._glob_snapshot, model._loc_snapshot,
              tuple(model.get_param_vector()))
    assert model.mean_gradient_labels == MEAN
    dev, md, rows = model._pack(c["P"], update_caches=False)
    raw = dev.loglike_mean_grad(md, rows, columns(dev, md, MEAN))
    lnl, g = model.log_likelihood_mean_gradient_batch(c["P"])
    np.testing.assert_array_equal(lnl, raw["lnl"])
    np.testing.assert_array_equal(g, raw["grad"])
    np.testing.assert_array_equal(lnl, model.log_likelihood_batch(c["P"]))
    lnl1, g1 = model.log_likelihood_mean_gradient()
    assert lnl1 == l0 and tuple(g1) == MEAN
    lnl, full = model.log_likelihood_full_gradient_batch(c["P"])
    labels = model.labels
    assert full.shape == (3, len(labels)) and labels == synth.LABELS
    np.testing.assert_array_equal(full[:, [labels.index(k) for k in MEAN]], g)
    lc, gc = model.log_likelihood_gradient_batch(c["P"])
    np.testing.assert_array_equal(full[:, [labels.index(k) for k in model.gradient_labels]], gc)
    np.testing.assert_array_equal(lnl, lc)
    model.freeze(["vsini", "cheb:1", "logg"])
    kept = tuple(k for k in MEAN if k not in ("vsini", "cheb:1", "logg"))
    assert model.mean_gradient_labels == kept
    keep = [i for i, k in enumerate(synth.LABELS) if k not in ("vsini", "cheb:1", "logg")]
    lnl, gk = model.log_likelihood_mean_gradient_batch(c["P"][:, keep])
    dev, md, rows = model._pack(c["P"][:, keep], update_caches=False)
    np.testing.assert_array_equal(gk, dev.loglike_mean_grad(md, rows, columns(dev, md, kept))["grad"])
    model.thaw(["vsini", "cheb:1", "logg"])
    assert (len(model.residuals), model._lnprob, model._log_scale, model._glob_snapshot, model._loc_snapshot,
            tuple(model.get_param_vector())) == before
    assert model.log_likelihood() == l0


def test_train_with_the_gradient_does_not_decrease_the_likelihood_and_leaves_the_model_at_the_solution():
    c = case("N256")
    model = synth.build_model(c["o"])
    model.set_param_vector(c["P"][0])
    start = model.log_likelihood()
    soln = model.train(gradient=True, options=dict(maxiter=3))
    print(f"train(gradient=True, maxiter=3): {soln.message}; nit {soln.nit}, nfev {soln.nfev}; lnL {start!r} -> {-soln.fun!r}")
    assert soln.x.shape == (len(model.labels),) and -soln.fun >= start
    np.testing.assert_array_equal(model.get_param_vector(), soln.x)
    assert model.log_likelihood() == -soln.fun
