"""The likelihood gradient in the mean-flux parameters without a device: (a) the numpy helper of the GPU test
(tests/mean_derivatives.py) against Richardson-extrapolated central differences of the oracle's likelihood, (b) each of its
tangents alone against central differences of the oracle's emulator_terms, (c) the power series of sb' that the device uses
below u = 2 against np.longdouble across the switch point, and the coefficient table in the kernel source, (d) the refusals
of sf_loglike_mean_grad_batch that need no context and the model methods over a stand-in DeviceOrder.

The criterion of (a) and (b) calibrates itself: with d(h) the central difference quotient at step h and R = (4 d(h/2) - d(h)) / 3,
the analytic value has to lie within 4 |d(h) - d(h/2)| of R (|d(h) - d(h/2)| is three times the h^2 term that R removes, so
what R keeps wrong is far below it unless the step is badly chosen), plus 1e-13 S_q for the rounding of the sums.  The steps
are chosen so that d(h) and d(h/2) agree to 1e-6 (|g| + 1) in every slot, which the test asserts as a condition."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import sf_oracle as O
from starfish_amd import _lib, synth

import mean_derivatives as MD
from gpu_helpers import oracle_order
from stand_in import StandIn as HostStandIn, model_on_a_stand_in, state_of

SF_EINVAL = -1
FAKE = 0x10000
LD = np.longdouble
MEAN = tuple(k for k in synth.LABELS if not k.startswith(("global_cov", "local_cov")))
STEPS = {"vz": 1e-2, "vsini": 1e-2, "log_scale": 3e-5, "cheb:1": 1e-4, "cheb:2": 1e-4, "T": 1e-1, "logg": 1e-3, "Z": 1e-3}


def richardson(f, x, h):
    d1 = (f(x + h) - f(x - h)) / (2 * h)
    d2 = (f(x + h / 2) - f(x - h / 2)) / h
    return (4 * d2 - d1) / 3, np.abs(d1 - d2)


_ORDERS = {}


def order(N):
    if N not in _ORDERS:
        o = synth.make_order(N=N, m=4, seed=5)
        _ORDERS[N] = (o, oracle_order(o), synth.walker_ball(o, B=3, seed=3))
    return _ORDERS[N]


# ------------------------------------------------------------------ (a) the helper's gradient
@pytest.mark.parametrize("N", [180, 330])
def test_helper_gradient_agrees_with_richardson_differences_of_the_oracles_likelihood(N):
    o, oo, P = order(N)
    assert MEAN == ("vz", "vsini", "log_scale", "cheb:1", "cheb:2", "T", "logg", "Z")
    for b, vec in enumerate(P):
        got = MD.gradient(oo, synth.vector_to_oracle_params(vec), MEAN)
        for name in MEAN:
            i = synth.LABELS.index(name)

            def lnl(x):
                v = vec.copy()
                v[i] = x
                return O.log_likelihood(oo, synth.vector_to_oracle_params(v))

            ref, spread = richardson(lnl, vec[i], STEPS[name])
            g, sq = got[name]
            print(f"N {N} walker {b} {name}: helper {g!r}, S_q {sq:.3g}, Richardson {ref!r}, |d(h) - d(h/2)| {spread:.3g}, "
                  f"|helper - R| / that {abs(g - ref) / spread:.3g}")
            assert spread <= 1e-6 * (abs(g) + 1), (N, b, name, spread)
            assert abs(g - ref) <= 4 * spread + 1e-13 * sq, (N, b, name, g, ref, spread)


# ------------------------------------------------------------------ (b) each tangent alone
def test_every_tangent_agrees_with_central_differences_of_emulator_terms():
    o, oo, P = order(180)
    vec = P[0]
    flux, X, S, tan = MD.tangents(oo, synth.vector_to_oracle_params(vec))
    f0, X0, S0, _ = O.emulator_terms(oo, synth.vector_to_oracle_params(vec))
    eps = np.finfo(np.float64).eps
    # (the helper evaluates the collocation spline, the oracle FITPACK's: rounding relative to the rows, which are of order 1)
    assert np.abs(flux - f0).max() <= 64 * eps and np.abs(X - X0).max() <= 64 * eps
    assert np.abs(S - S0).max() <= 64 * eps * np.abs(S0).max()
    for name in MEAN:
        i = synth.LABELS.index(name)

        def terms(x, pick):
            v = vec.copy()
            v[i] = x
            return O.emulator_terms(oo, synth.vector_to_oracle_params(v))[pick]

        kind, d0, d1 = tan[name]
        # rows: (df, dX); grid: (dmu, dS), where the flux moves by dmu^T X and X stays
        pairs = [("flux", 0, d0 if kind == "rows" else d0 @ X), ("X", 1, d1 if kind == "rows" else np.zeros_like(X)),
                 ("Sigma_w", 2, np.zeros_like(S) if kind == "rows" else d1)]
        for what, pick, got in pairs:
            ref, spread = richardson(lambda x: terms(x, pick), vec[i], STEPS[name])
            size = max(np.abs(got).max(), np.abs(ref).max())
            tol = 4 * spread.max() + 1e-13 * np.abs(terms(vec[i], pick)).max() / STEPS[name]
            err = np.abs(got - ref).max()
            print(f"{name} d {what}: max |tangent| {size:.3g}, max |tangent - R| {err:.3g}, allowed {tol:.3g}")
            assert err <= tol, (name, what, err, tol)


# ------------------------------------------------------------------ (c) the series of sb'
def kernel_table():
    src = open(os.path.join(os.path.dirname(__file__), "..", "starfish_amd", "csrc", "sf_mean_grad.h")).read()
    body = re.search(r"const double c\[12\] = \{(.*?)\};", src, re.S).group(1)
    switch = float(re.search(r"#define SF_ROT_DSERIES_U ([0-9.]+)", src).group(1))
    return np.array([float(v) for v in body.replace("\n", " ").split(",")]), switch


def test_kernel_series_table_holds_the_coefficients_and_the_switch_point_of_the_helper():
    table, switch = kernel_table()
    want = np.array([float((-1) ** k * 2 * k * MD._series_coefficient(k)) for k in range(12, 0, -1)])
    np.testing.assert_array_equal(table, want)
    assert switch == MD.SERIES_U == 2.0


def test_sb_prime_series_and_closed_form_against_longdouble_across_the_switch_point():
    """u sb'(u) as the kernel forms it (12 terms by Horner in float64 below u = 2, the closed form above) against 40 terms in
    longdouble: both within 8 eps relative on their side of the switch; one step further (the series up to 2.5, the closed form
    down to 1.5) each is still within 16 eps, so the choice of the switch point is not delicate."""
    table, switch = kernel_table()
    eps = np.finfo(np.float64).eps

    def horner(u):
        s = np.zeros_like(u)
        for c in table:
            s = s * (u * u) + c
        return s * (u * u)

    below, above = np.linspace(1e-3, switch, 4001)[:-1], np.linspace(switch, 3.0, 2001)
    ref = lambda u: (MD.sb_prime_series(u) * u.astype(LD))  # noqa: E731
    rel = lambda got, u: float(np.max(np.abs((got - ref(u)) / ref(u))))  # noqa: E731
    e_series, e_closed = rel(horner(below), below), rel(MD.sb_prime_closed(above) * above, above)
    wide = np.linspace(switch, 2.5, 1001)
    low = np.linspace(1.5, switch, 1001)
    e_series_wide, e_closed_low = rel(horner(wide), wide), rel(MD.sb_prime_closed(low) * low, low)
    print(f"series below {switch}: {e_series / eps:.2f} eps; closed form above: {e_closed / eps:.2f} eps; series on [2, 2.5]: "
          f"{e_series_wide / eps:.2f} eps; closed form on [1.5, 2]: {e_closed_low / eps:.2f} eps; closed form at 0.25: "
          f"{rel(MD.sb_prime_closed(np.array([0.25])) * 0.25, np.array([0.25])) / eps:.0f} eps")
    assert e_series <= 8 * eps and e_closed <= 8 * eps
    assert e_series_wide <= 16 * eps and e_closed_low <= 16 * eps
    # the helper's own multiplier derivative against Richardson differences of rot_broaden's multiplier
    wave = np.exp(np.linspace(np.log(5000.0), np.log(5010.0), 512))
    ref, spread = richardson(lambda v: MD.rot_multipliers(wave, 512, v)[0], 30.0, 1e-2)
    assert np.abs(MD.rot_multipliers(wave, 512, 30.0)[1] - ref).max() <= 4 * spread.max() + 1e-13


# ------------------------------------------------------------------ (d) refusals without a context, the model methods
GOOD = dict(ctx=None, B=4, params=FAKE, slots=(C.c_int * 2)(1, 2), nslots=2, lnl=FAKE + (1 << 20), grad=FAKE + (1 << 21),
            grad_stride=2, flux=None, info=None, work=FAKE + (1 << 28), work_bytes=1 << 20)
BAD = {
    "no walker": dict(B=0),
    "more walkers than a grid plane": dict(B=65536),
    "null params": dict(params=None),
    "null slots": dict(slots=None),
    "null lnl": dict(lnl=None),
    "null grad": dict(grad=None),
}


def mean_grad(lib, md, **kw):
    a = dict(GOOD, **kw)
    return lib.sf_loglike_mean_grad_batch(a["ctx"], md, a["B"], a["params"], a["slots"], a["nslots"], a["lnl"], a["grad"],
                                          a["grad_stride"], a["flux"], a["info"], a["work"], a["work_bytes"], None)


@pytest.mark.parametrize("case", list(BAD))
def test_mean_grad_refuses_bad_arguments_before_it_looks_at_the_context(case):
    lib = _lib.load()
    md = _lib.ModelDesc()
    md.has_log_scale = md.has_vz = 1
    rc = mean_grad(lib, C.byref(md), **BAD[case])
    assert rc == SF_EINVAL, (case, rc)
    assert lib.sf_last_error().decode().startswith("sf_loglike_mean_grad_batch:"), (case, lib.sf_last_error())


def test_mean_grad_entry_points_are_present():
    lib = _lib.load()
    for name in ("sf_loglike_mean_grad_workspace_bytes", "sf_loglike_mean_grad_batch", "sf_debug_loglike_mean_grad_contract"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    md = _lib.ModelDesc()
    md.has_log_scale = 1
    assert mean_grad(lib, C.byref(md)) == SF_EINVAL
    assert lib.sf_last_error().decode() == "bad context / model descriptor"
    assert lib.sf_loglike_mean_grad_workspace_bytes(None, C.byref(md), 4, 2) == 0


class StandIn(HostStandIn):
    """What SpectrumModel asks of a DeviceOrder here; the gradients name their walker and their slot (covariance) or column."""

    def loglike_grad(self, md, rows, want_flux=False, max_chunk=None):
        B, slots = rows.shape[0], (2 if md.has_global else 0) + 3 * md.n_local
        self.calls.append(("cov", B, slots))
        b, s = np.meshgrid(np.arange(B), np.arange(slots), indexing="ij")
        return dict(lnl=-100.0 - np.arange(B), grad=10.0 * b + s + 0.25, info=np.full(B, self.info, dtype=np.int32))

    def loglike_mean_grad(self, md, rows, slots, want_flux=False, max_chunk=None):
        B = rows.shape[0]
        self.calls.append(("mean", B, tuple(slots)))
        self.rows = rows.copy()
        # a concave bowl around 1 in every column asked for: lnL = -100 - b - 1/2 sum (x - 1)^2
        x = rows[:, list(slots)]
        return dict(lnl=-100.0 - np.arange(B) - 0.5 * ((x - 1) ** 2).sum(axis=1), grad=-(x - 1),
                    info=np.full(B, self.info, dtype=np.int32))


def test_mean_gradient_labels_and_columns_follow_what_is_thawed():
    model, dev = model_on_a_stand_in(StandIn, params=dict(Av=0.2, Rv=3.1))
    assert model.labels[:3] == ("vz", "vsini", "log_scale") and "Rv" in model.labels and "Av" in model.labels
    every = tuple(k for k in model.labels if not k.startswith(("global_cov", "local_cov")) and k != "Rv")
    assert model.mean_gradient_labels == every and set(every) == set(MEAN) | {"Av"}
    assert model.gradient_labels == tuple(k for k in model.labels if k.startswith(("global_cov", "local_cov")))
    column = {"vsini": 0, "vz": 1, "log_scale": 2, "T": 6, "logg": 7, "Z": 8, "cheb:1": 9, "cheb:2": 10, "Av": 14}
    state = state_of(model)
    lnl, grad = model.log_likelihood_mean_gradient()
    assert dev.calls[-1] == ("mean", 1, tuple(column[k] for k in every)) and tuple(grad) == every
    x = dict(zip(model.labels, model.get_param_vector()))
    assert list(grad.values()) == [-(x[k] - 1) for k in every]
    P = np.tile(model.get_param_vector(), (3, 1))
    lnl, g, info = model.log_likelihood_mean_gradient_batch(P, return_info=True)
    assert lnl.shape == (3,) and g.shape == (3, len(every)) and (info == 0).all()
    lnl, full = model.log_likelihood_full_gradient_batch(P)
    assert full.shape == (3, len(model.labels)) and [c[0] for c in dev.calls[-2:]] == ["mean", "cov"]
    np.testing.assert_array_equal(full[:, [model.labels.index(k) for k in every]], g)
    np.testing.assert_array_equal(full[:, [model.labels.index(k) for k in model.gradient_labels]],
                                  10.0 * np.arange(3)[:, None] + np.arange(5)[None, :] + 0.25)
    assert (full[:, model.labels.index("Rv")] == 0).all()
    assert state_of(model) == state
    model.freeze(["vsini", "T", "cheb:1", "global_cov"])
    kept = tuple(k for k in every if k not in ("vsini", "T", "cheb:1"))
    assert model.mean_gradient_labels == kept
    lnl, grad = model.log_likelihood_mean_gradient()
    assert dev.calls[-1] == ("mean", 1, tuple(column[k] for k in kept)) and tuple(grad) == kept
    model.freeze([k for k in model.labels if not k.startswith("local_cov")])
    assert model.mean_gradient_labels == ()
    n = len(dev.calls)
    with pytest.raises(ValueError, match="no thawed mean-flux parameter"):
        model.log_likelihood_mean_gradient()
    lnl, full = model.log_likelihood_full_gradient_batch(np.tile(model.get_param_vector(), (2, 1)))
    assert full.shape == (2, 3) and [c[0] for c in dev.calls[n:]] == ["cov"]


def test_models_the_device_does_not_differentiate_are_refused_with_a_reason():
    o = synth.make_order(N=64, m=3, seed=9)
    params = synth.centre_params(o)
    del params["log_scale"]
    model = synth.build_model(o, params=params)
    model._device = lambda: StandIn(64)
    with pytest.raises(ValueError, match="log_scale"):
        model.log_likelihood_mean_gradient()
    model, dev = model_on_a_stand_in(StandIn, emulator_cov="paper")
    with pytest.raises(ValueError, match="paper"):
        model.log_likelihood_mean_gradient_batch(np.tile(model.get_param_vector(), (2, 1)))
    with pytest.raises(ValueError, match="paper"):
        model.train(gradient=True)
    model, dev = model_on_a_stand_in(StandIn)
    model.norm = True
    with pytest.raises(ValueError, match="norm=True"):
        model.log_likelihood_mean_gradient()
    assert dev.calls == []
    model.emulator.norm_factor = lambda g: np.ones(len(np.atleast_2d(g)))
    model.freeze(["T", "logg", "Z"])
    model.log_likelihood_mean_gradient()
    assert dev.calls[-1][0] == "mean"
    dev.info = -1
    with pytest.raises(ValueError, match="outside of original parameter range"):
        model.log_likelihood_mean_gradient()
    dev.info = 7
    with pytest.raises(np.linalg.LinAlgError, match="7-th leading minor"):
        model.train(gradient=True)


def test_train_gradient_runs_lbfgsb_over_all_labels_and_leaves_the_model_at_the_solution():
    model, dev = model_on_a_stand_in(StandIn, freeze=("global_cov", "local_cov"))
    labels = model.labels
    assert labels == model.mean_gradient_labels and len(labels) == 8

    class Normal:
        def __init__(self, at):
            self.at = at

        def logpdf(self, x):
            return -0.5 * (np.asarray(x) - self.at) ** 2

    with pytest.raises(ValueError, match="Invalid priors"):
        model.train(gradient=True, priors={"nonsense": Normal(0.0)})
    assert dev.calls == []
    soln = model.train(gradient=True, priors={"vz": Normal(3.0)})
    assert soln.success and soln.x.shape == (8,) and soln.nfev == len(dev.calls)
    want = np.ones(8)
    want[labels.index("vz")] = 2.0  # the bowl around 1 and the prior around 3 meet half way
    np.testing.assert_allclose(soln.x, want, atol=1e-5)
    np.testing.assert_array_equal(model.get_param_vector(), soln.x)
    assert all(call[0] == "mean" and call[1] == 1 for call in dev.calls)
    # the default path is the Nelder-Mead loop as before: it never asks for a gradient
    model2, dev2 = model_on_a_stand_in(StandIn)
    assert model2.train.__defaults__ == (None, True, False)
