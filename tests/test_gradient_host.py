"""The likelihood gradient in the covariance hyper-parameters without a device: (a) the numpy helper of the GPU test
(tests/cov_derivatives.py) against the oracle's kernels and against a 5-point stencil of its own values in longdouble, (b) the
identity d lnL / d theta = 1/2 sum (alpha alpha^T - C^-1) o dC/dtheta (Rasmussen & Williams, GPML, eq. 5.9) in the oracle
against central differences of its likelihood, (c) the refusals of sf_loglike_grad_batch / sf_potri_blocks_batch that need no
context, and (d) the model methods over a stand-in DeviceOrder."""
import ctypes as C

import numpy as np
import pytest

from oracle import sf_oracle as O
from starfish_amd import _lib, synth

import cov_derivatives as CD
from stand_in import StandIn as HostStandIn, model_on_a_stand_in, state_of

SF_EINVAL = -1
FAKE = 0x10000  # a non-null "device pointer": a refused call never touches it
LD = np.longdouble
N = 180


def order():
    return synth.make_order(N=N, m=4, seed=5)


def stencil(f, x, h):
    """5-point first derivative: truncation h^4 / 30 |f^(5)|."""
    return (-f(x + 2 * h) + 8 * f(x + h) - 8 * f(x - h) + f(x - 2 * h)) / (12 * h)


# ------------------------------------------------------------------ (a) the helper
def centre(o):
    c = synth.centre_params(o)
    w = o["wave"]
    k = N // 3
    mu = w[k] + 0.3 * (w[k + 1] - w[k])  # 0.3 pixel off a pixel: no kink within the stencil
    return c["global_cov"]["log_amp"], c["global_cov"]["log_ls"], mu, c["local_cov"][0]["log_amp"], c["local_cov"][0]["log_sigma"]


def test_helper_values_equal_the_oracles_kernels():
    o = order()
    la, ll, mu, lla, lls = centre(o)
    w = o["wave"]
    eps = np.finfo(np.float64).eps
    for got, ref in ((CD.global_kernel(w, la, ll)["K"], O.matern32_global(w, np.exp(la), np.exp(ll))),
                     (CD.local_kernel(w, mu, lla, lls)["K"], O.gaussian_local(w, np.exp(lla), mu, np.exp(lls)))):
        assert got.dtype == np.float64 and (ref != 0).sum() > N
        np.testing.assert_array_equal(got == 0, ref == 0)
        np.testing.assert_allclose(got, ref, rtol=4 * eps, atol=0)
    assert CD.global_kernel(w.astype(LD), LD(la), LD(ll))["log_ls"].dtype == LD
    assert CD.local_kernel(w.astype(LD), LD(mu), LD(lla), LD(lls))["mu"].dtype == LD


def test_helper_derivatives_agree_with_a_stencil_of_its_own_values():
    """Tolerance 1e-8 max|D|: the stencil's truncation at relative step 1e-3 is about 1e-12, a missing term is an error of
    order 1.  log_ls only: the second derivative of the taper jumps at the cut-off r = r0, so the stencil itself is O(h)
    for entries with |r / r0 - 1| < 3 h; they are left out (at most 1 % of the entries) and shown to converge with h."""
    o = order()
    la, ll, mu, lla, lls = (LD(v) for v in centre(o))
    w = o["wave"].astype(LD)
    h = LD(1e-3)
    pix = w[N // 3 + 1] - w[N // 3]
    cases = [
        ("global log_amp", CD.global_kernel(w, la, ll)["log_amp"], lambda x: CD.global_kernel(w, x, ll)["K"], la, h),
        ("global log_ls", CD.global_kernel(w, la, ll)["log_ls"], lambda x: CD.global_kernel(w, la, x)["K"], ll, h),
        ("local mu", CD.local_kernel(w, mu, lla, lls)["mu"], lambda x: CD.local_kernel(w, x, lla, lls)["K"], mu, h * pix),
        ("local log_amp", CD.local_kernel(w, mu, lla, lls)["log_amp"], lambda x: CD.local_kernel(w, mu, x, lls)["K"], lla, h),
        ("local log_sigma", CD.local_kernel(w, mu, lla, lls)["log_sigma"], lambda x: CD.local_kernel(w, mu, lla, x)["K"], lls, h),
    ]
    for name, D, f, x, step in cases:
        assert D.dtype == LD and np.abs(D).max() > 0
        err = np.abs(stencil(f, x, step) - D)
        keep = np.ones(D.shape, dtype=bool)
        if name == "global log_ls":
            r = LD(CD.C_KMS) / 2 * np.abs((w[None, :] - w[:, None]) / (w[None, :] + w[:, None]))
            keep = np.abs(r / (6 * np.exp(ll)) - 1) >= 3 * h
            left_out = int((~keep).sum())
            assert 0 < left_out <= 0.01 * D.size, left_out
            finer = np.abs(stencil(f, x, step / 10) - D)
            worst, worst_finer = float(err[~keep].max()), float(finer[~keep].max())
            print(f"{name}: {left_out} of {D.size} entries at the cut-off left out; there the stencil is off by "
                  f"{worst / float(np.abs(D).max()):.3g} max|D| at h = 1e-3 and {worst_finer / float(np.abs(D).max()):.3g} at 1e-4")
            assert worst_finer < 0.5 * worst
        rel = float(err[keep].max() / np.abs(D).max())
        print(f"{name}: max |stencil - D| = {rel:.3g} max|D|")
        assert rel <= 1e-8, (name, rel)


# ------------------------------------------------------------------ (b) the identity, in the oracle
def test_the_contraction_is_the_gradient_of_the_oracles_likelihood():
    """1/2 sum A o D with numpy.linalg on the oracle's matrix plus jitter against central differences of the oracle's
    likelihood: steps 1e-4 in the log parameters and 1e-3 pixel in mu (the walkers' mu lie at least 0.06 pixel from the
    nearest kink)."""
    o = order()
    oo = O.OracleOrder(o["wave"], o["flux"], o["sigma"], o["emu_wl"], o["eigenspectra"], o["flux_mean"], o["flux_std"],
                       o["grid_points"], o["w_hat"])
    pix = o["wave"][N // 3 + 1] - o["wave"][N // 3]
    for b, vec in enumerate(synth.walker_ball(o, B=3, seed=3)):
        p = synth.vector_to_oracle_params(vec)
        flux, cov, _ = O.forward_model(oo, p)
        Cj = cov + O.JITTER * np.eye(N)
        alpha = np.linalg.solve(Cj, flux - oo.flux)
        A = np.outer(alpha, alpha) - np.linalg.inv(Cj)
        for name, D in CD.slot_derivatives(o["wave"], p):
            got = 0.5 * np.sum(A * D)
            i = synth.LABELS.index(name)
            step = 1e-3 * pix if name.endswith(":mu") else 1e-4

            def lnl(x):
                v = vec.copy()
                v[i] = x
                return O.log_likelihood(oo, synth.vector_to_oracle_params(v))

            fd = (lnl(vec[i] + step) - lnl(vec[i] - step)) / (2 * step)
            rel = abs(got - fd) / abs(fd)
            print(f"walker {b} {name}: contraction {got:.12g}, central difference {fd:.12g}, relative {rel:.3g}")
            assert rel <= 1e-6, (b, name, got, fd)


# ------------------------------------------------------------------ (c) refusals
GRAD_GOOD = dict(ctx=None, B=4, params=FAKE, lnl=FAKE + (1 << 20), grad=FAKE + (1 << 21), grad_stride=5, flux=None, info=None,
                 work=FAKE + (1 << 28), work_bytes=1 << 20)
GRAD_BAD = {
    "no walker": dict(B=0),
    "negative batch": dict(B=-3),
    "more walkers than a grid plane": dict(B=65536),
    "null params": dict(params=None),
    "null lnl": dict(lnl=None),
    "null grad": dict(grad=None),
    "gradient rows shorter than the slots": dict(grad_stride=4),
}


def model_desc(has_global=1, n_local=1):
    md = _lib.ModelDesc()
    md.has_global, md.n_local = has_global, n_local
    return md


def loglike_grad(lib, md, **kw):
    a = dict(GRAD_GOOD, **kw)
    return lib.sf_loglike_grad_batch(a["ctx"], md, a["B"], a["params"], a["lnl"], a["grad"], a["grad_stride"], a["flux"],
                                     a["info"], a["work"], a["work_bytes"], None)


@pytest.mark.parametrize("case", list(GRAD_BAD))
def test_loglike_grad_refuses_bad_arguments_before_it_looks_at_the_context(case):
    lib = _lib.load()
    rc = loglike_grad(lib, C.byref(model_desc()), **GRAD_BAD[case])
    assert rc == SF_EINVAL, (case, rc)
    assert lib.sf_last_error().decode().startswith("sf_loglike_grad_batch:"), (case, lib.sf_last_error())


def test_loglike_grad_entry_points_are_present_and_refuse_what_they_cannot_differentiate():
    lib = _lib.load()
    for name in ("sf_loglike_grad_workspace_bytes", "sf_loglike_grad_batch", "sf_potri_blocks_workspace_bytes",
                 "sf_potri_blocks_batch"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert loglike_grad(lib, C.byref(model_desc(0, 0))) == SF_EINVAL
    msg = lib.sf_last_error().decode()
    assert msg.startswith("sf_loglike_grad_batch:") and "nothing to differentiate" in msg
    for md in (C.byref(model_desc()), None):
        assert loglike_grad(lib, md) == SF_EINVAL
        assert lib.sf_last_error().decode() == "bad context / model descriptor"
    assert lib.sf_loglike_grad_workspace_bytes(None, C.byref(model_desc()), 4) == 0
    assert lib.sf_loglike_grad_workspace_bytes(None, C.byref(model_desc()), 0) == 0


BLOCKS_BYTES = 3 * 2 * 64 * 64 * 8 + 3 * 128 * 8
BLOCKS_GOOD = dict(L=FAKE, n=128, lda=144, stride=128 * 144, batch=3, pairs=FAKE + (1 << 20), npairs=3, out=FAKE + (1 << 24),
                   work=FAKE + (1 << 28), work_bytes=BLOCKS_BYTES)
BLOCKS_BAD = {
    "order zero": dict(n=0),
    "negative order": dict(n=-64),
    "order not a multiple of 64": dict(n=96),
    "rows shorter than the order": dict(lda=127),
    "no matrix": dict(batch=0),
    "no pair": dict(npairs=0),
    "null factor": dict(L=None),
    "null pairs": dict(pairs=None),
    "null result": dict(out=None),
    "null workspace": dict(work=None),
    "workspace a byte short": dict(work_bytes=BLOCKS_BYTES - 1),
}


@pytest.mark.parametrize("case", list(BLOCKS_BAD))
def test_potri_blocks_refuses_bad_arguments_before_any_device_call(case):
    lib = _lib.load()
    assert lib.sf_potri_blocks_workspace_bytes(128, 3) == BLOCKS_BYTES
    a = dict(BLOCKS_GOOD, **BLOCKS_BAD[case])
    rc = lib.sf_potri_blocks_batch(a["L"], a["n"], a["lda"], a["stride"], a["batch"], a["pairs"], a["npairs"], a["out"], a["work"],
                                   a["work_bytes"], None)
    assert rc == SF_EINVAL, (case, rc)
    assert lib.sf_last_error().decode().startswith("sf_potri_blocks_batch:"), (case, lib.sf_last_error())
    assert lib.sf_potri_blocks_workspace_bytes(0, 3) == 0 and lib.sf_potri_blocks_workspace_bytes(128, 0) == 0
    assert lib.sf_potri_blocks_workspace_bytes(96, 3) == 0


# ------------------------------------------------------------------ (d) the model methods over a stand-in DeviceOrder
class StandIn(HostStandIn):
    """What SpectrumModel asks of a DeviceOrder here; loglike_grad returns numbers that name their walker and slot."""

    def loglike_grad(self, md, rows, want_flux=False, max_chunk=None):
        B, slots = rows.shape[0], (2 if md.has_global else 0) + 3 * md.n_local
        self.calls.append((B, slots))
        b, s = np.meshgrid(np.arange(B), np.arange(slots), indexing="ij")
        return dict(lnl=-100.0 - np.arange(B), grad=10.0 * b + s + 0.25, info=np.full(B, self.info, dtype=np.int32))


def two_local(o):
    params = synth.centre_params(o)
    params["local_cov"] = params["local_cov"] + [dict(mu=float(o["wave"][40]), log_amp=-8.5, log_sigma=2.5)]
    return params


def test_gradient_labels_follow_what_is_thawed():
    model, dev = model_on_a_stand_in(StandIn, params=two_local)
    every = ("global_cov:log_amp", "global_cov:log_ls", "local_cov:0:mu", "local_cov:0:log_amp", "local_cov:0:log_sigma",
             "local_cov:1:mu", "local_cov:1:log_amp", "local_cov:1:log_sigma")
    assert model.gradient_labels == every
    state = state_of(model)
    lnl, grad = model.log_likelihood_gradient()
    assert lnl == -100.0 and tuple(grad) == every
    assert list(grad.values()) == [s + 0.25 for s in range(8)]
    P = np.tile(model.get_param_vector(), (3, 1))
    lnl, g = model.log_likelihood_gradient_batch(P)
    assert lnl.shape == (3,) and g.shape == (3, 8)
    np.testing.assert_array_equal(g, 10.0 * np.arange(3)[:, None] + np.arange(8)[None, :] + 0.25)
    lnl, g, info = model.log_likelihood_gradient_batch(P, return_info=True)
    assert info.shape == (3,) and (info == 0).all()
    assert state_of(model) == state
    # individually frozen labels leave their columns out; the device still differentiates in every slot
    model.freeze(["local_cov:0:mu", "global_cov:log_ls", "vz"])
    kept = ("global_cov:log_amp", "local_cov:0:log_amp", "local_cov:0:log_sigma", "local_cov:1:mu", "local_cov:1:log_amp",
            "local_cov:1:log_sigma")
    assert model.gradient_labels == kept
    lnl, grad = model.log_likelihood_gradient()
    assert tuple(grad) == kept and list(grad.values()) == [0.25, 3.25, 4.25, 5.25, 6.25, 7.25]
    P = np.tile(model.get_param_vector(), (2, 1))
    lnl, g = model.log_likelihood_gradient_batch(P)
    assert g.shape == (2, 6)
    np.testing.assert_array_equal(g[1], 10.0 + np.array([0.25, 3.25, 4.25, 5.25, 6.25, 7.25]))
    # a frozen group leaves all of its labels out
    model.freeze("local_cov")
    assert model.gradient_labels == ("global_cov:log_amp",)
    lnl, g = model.log_likelihood_gradient_batch(np.tile(model.get_param_vector(), (2, 1)))
    assert g.shape == (2, 1) and list(g[:, 0]) == [0.25, 10.25]
    assert all(call[1] == 8 for call in dev.calls)


def test_nothing_thawed_is_a_value_error_and_failures_raise_as_the_likelihood_does():
    model, dev = model_on_a_stand_in(StandIn)
    P = np.tile(model.get_param_vector(), (3, 1))
    with pytest.raises(ValueError):
        model.log_likelihood_gradient_batch(P[:, :-1])
    dev.info = -1
    with pytest.raises(ValueError, match="outside of original parameter range"):
        model.log_likelihood_gradient()
    dev.info = 7
    with pytest.raises(np.linalg.LinAlgError, match="7-th leading minor"):
        model.log_likelihood_gradient()
    lnl, g, info = model.log_likelihood_gradient_batch(P, return_info=True)  # the batch reports instead
    assert (info == 7).all() and np.isneginf(lnl).all()
    with pytest.raises(np.linalg.LinAlgError):
        model.train_covariance()
    dev.info = 0
    model.freeze(["global_cov", "local_cov"])
    assert model.gradient_labels == ()
    calls = len(dev.calls)
    for call in (model.log_likelihood_gradient, lambda: model.log_likelihood_gradient_batch(np.zeros((2, len(model.labels)))),
                 model.train_covariance):
        with pytest.raises(ValueError):
            call()
    assert len(dev.calls) == calls


def test_train_covariance_checks_its_priors_as_train_does():
    model, dev = model_on_a_stand_in(StandIn)

    class Flat:
        def logpdf(self, x):
            return 0.0 * np.asarray(x)

    with pytest.raises(ValueError, match="Invalid priors"):
        model.train_covariance(priors={"nonsense": Flat()})
    with pytest.raises(ValueError, match="logpdf"):
        model.train_covariance(priors={"global_cov:log_amp": 1.0})
    assert dev.calls == []
