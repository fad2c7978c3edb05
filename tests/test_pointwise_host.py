"""The per-pixel leave-one-out diagnostics without a device: the refusals of sf_pointwise_batch / sf_potri_diag_batch that
need no context (SF_EINVAL and a message before any HIP call; what follows the context check is in
tests/test_gpu_pointwise.py), the Python-side shape checks and formulas of SpectrumModel.pointwise / pointwise_batch with a
stand-in DeviceOrder, and the identity the feature rests on, in the oracle."""
import ctypes as C

import numpy as np
import pytest

from oracle import sf_oracle as O
from starfish_amd import _lib, synth
from starfish_amd.models import SpectrumModel

from stand_in import StandIn as HostStandIn, model_on_a_stand_in

SF_EINVAL = -1
FAKE = 0x10000  # a non-null "device pointer": a refused call never touches it
U = 2.0 ** -53
DERIVED = ("alpha", "marginal_std", "loo_mean", "loo_std", "z", "log_density")


def gamma(k):
    return k * U / (1 - k * U)


GOOD = dict(ctx=None, B=4, params=FAKE, rhs=FAKE + (1 << 20), nrhs=3, ldr=4096, rhs_stride=3 * 4096, alpha=FAKE + (1 << 24),
            cinv_diag=FAKE + (1 << 25), cov_diag=None, flux=None, info=None, work=FAKE + (1 << 28), work_bytes=1 << 20)

# refused on the counts, the pointers and the right-hand-side conventions: before the context is looked at
BAD = {
    "no walker": dict(B=0),
    "negative batch": dict(B=-3),
    "more walkers than a grid plane": dict(B=65536),
    "no right-hand side": dict(nrhs=0),
    "more right-hand sides than a grid row": dict(nrhs=65536),
    "null params": dict(params=None),
    "null alpha": dict(alpha=None),
    "null cinv_diag": dict(cinv_diag=None),
    "negative rhs stride": dict(rhs_stride=-1),
    "the residual as two right-hand sides": dict(rhs=None, nrhs=2),
}


def pointwise(lib, md, **kw):
    a = dict(GOOD, **kw)
    return lib.sf_pointwise_batch(a["ctx"], md, a["B"], a["params"], a["rhs"], a["nrhs"], a["ldr"], a["rhs_stride"], a["alpha"],
                                  a["cinv_diag"], a["cov_diag"], a["flux"], a["info"], a["work"], a["work_bytes"], None)


@pytest.mark.parametrize("case", list(BAD))
def test_pointwise_refuses_bad_arguments_before_it_looks_at_the_context(case):
    lib = _lib.load()  # loading needs no GPU; a call that reached the HIP runtime here would not return SF_EINVAL
    rc = pointwise(lib, C.byref(_lib.ModelDesc()), **BAD[case])
    assert rc == SF_EINVAL, (case, rc)
    msg = lib.sf_last_error().decode()
    assert msg.startswith("sf_pointwise_batch:"), (case, msg)


def test_pointwise_entry_points_refuse_a_missing_context_or_model():
    lib = _lib.load()
    md = _lib.ModelDesc()
    for name in ("sf_pointwise_workspace_bytes", "sf_pointwise_batch", "sf_potri_diag_workspace_bytes", "sf_potri_diag_batch"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.sf_pointwise_workspace_bytes(None, C.byref(md), 4, 1) == 0
    assert lib.sf_pointwise_workspace_bytes(None, C.byref(md), 0, 1) == 0
    assert lib.sf_pointwise_workspace_bytes(None, C.byref(md), 4, 0) == 0
    for model in (C.byref(md), None):
        assert pointwise(lib, model) == SF_EINVAL
        assert lib.sf_last_error().decode() == "bad context / model descriptor"
        assert pointwise(lib, model, rhs=None, nrhs=1, ldr=0, rhs_stride=0) == SF_EINVAL


POTRI_GOOD = dict(L=FAKE, n=128, lda=144, stride=128 * 144, batch=3, out=FAKE + (1 << 24), out_stride=128, work=FAKE + (1 << 28),
                  work_bytes=3 * 2 * 64 * 64 * 8)
POTRI_BAD = {
    "order zero": dict(n=0),
    "negative order": dict(n=-64),
    "order not a multiple of 64": dict(n=96),
    "rows shorter than the order": dict(lda=127),
    "no matrix": dict(batch=0),
    "results closer than the order": dict(out_stride=127),
    "null factor": dict(L=None),
    "null result": dict(out=None),
    "null workspace": dict(work=None),
    "workspace a byte short": dict(work_bytes=3 * 2 * 64 * 64 * 8 - 1),
}


@pytest.mark.parametrize("case", list(POTRI_BAD))
def test_potri_diag_refuses_bad_arguments_before_any_device_call(case):
    lib = _lib.load()
    assert lib.sf_potri_diag_workspace_bytes(128, 3) == POTRI_GOOD["work_bytes"]
    a = dict(POTRI_GOOD, **POTRI_BAD[case])
    rc = lib.sf_potri_diag_batch(a["L"], a["n"], a["lda"], a["stride"], a["batch"], a["out"], a["out_stride"], a["work"],
                                 a["work_bytes"], None)
    assert rc == SF_EINVAL, (case, rc)
    assert lib.sf_last_error().decode().startswith("sf_potri_diag_batch:"), (case, lib.sf_last_error())
    assert lib.sf_potri_diag_workspace_bytes(0, 3) == 0 and lib.sf_potri_diag_workspace_bytes(128, 0) == 0
    assert lib.sf_potri_diag_workspace_bytes(96, 3) == 0


# ------------------------------------------------------------------ the model methods over a stand-in DeviceOrder
class StandIn(HostStandIn):
    """What SpectrumModel asks of a DeviceOrder here; pointwise returns numbers that name their own index."""

    def pointwise(self, md, rows, rhs=None, want_flux=False, max_chunk=None):
        B, nrhs = rows.shape[0], 1 if rhs is None else rhs.shape[-2]
        self.calls.append((B, None if rhs is None else rhs.shape, want_flux))
        b, r, i = np.meshgrid(np.arange(B), np.arange(nrhs), np.arange(self.n), indexing="ij")
        out = dict(alpha=1e3 * b + 1e2 * r + i + 0.5, cinv_diag=4.0 + b[:, 0] + i[:, 0] / 64.0,
                   cov_diag=9.0 + 2.0 * b[:, 0] + i[:, 0] / 32.0, info=np.full(B, self.info, dtype=np.int32))
        if want_flux:
            out["flux"] = 7.0 * (b[:, 0] + 1) + i[:, 0]
        return out


def expected(model, B, rhs, N=64):
    """The formulas of the leave-one-out predictive on the stand-in's numbers; rhs None, (k, N) or (B, k, N)."""
    dev = StandIn(N)
    raw = dev.pointwise(None, np.zeros((B, 1)), rhs=rhs, want_flux=True)
    r = (raw["flux"] - model.data.flux)[:, None, :] if rhs is None else np.broadcast_to(rhs, raw["alpha"].shape)
    a, d = raw["alpha"], raw["cinv_diag"][:, None, :]
    z = a / np.sqrt(d)
    return dict(alpha=a, marginal_std=np.sqrt(raw["cov_diag"]), loo_mean=r - a / d, loo_std=1.0 / np.sqrt(raw["cinv_diag"]),
                z=z, log_density=-0.5 * np.log(2.0 * np.pi / d) - 0.5 * z * z)


def test_keys_shapes_and_formulas_of_the_model_methods():
    model, dev = model_on_a_stand_in(StandIn)
    N = 64
    state = (len(model.residuals), model._lnprob, model._log_scale, model._glob_snapshot, model._loc_snapshot)
    rng = np.random.default_rng(0)
    for rhs, lead in ((None, ()), (rng.standard_normal(N), ()), (rng.standard_normal((2, N)), (2,))):
        got = model.pointwise(rhs)
        want = expected(model, 1, None if rhs is None else np.atleast_2d(rhs))
        assert tuple(got) == DERIVED
        for key in DERIVED:
            per_matrix = key in ("marginal_std", "loo_std")
            assert got[key].shape == (() if per_matrix else lead) + (N,), key
            np.testing.assert_array_equal(got[key], want[key][0] if per_matrix or lead else want[key][0, 0], err_msg=key)
    assert dev.calls == [(1, None, True), (1, (1, N), False), (1, (2, N), False)]
    P = np.tile(model.get_param_vector(), (3, 1))
    for rhs, lead in ((None, ()), (rng.standard_normal(N), ()), (rng.standard_normal((2, N)), (2,)),
                      (rng.standard_normal((3, 2, N)), (2,))):
        got, info = model.pointwise_batch(P, rhs, return_info=True)
        want = expected(model, 3, None if rhs is None else rhs if rhs.ndim == 3 else np.atleast_2d(rhs))
        assert tuple(got) == DERIVED and info.shape == (3,)
        for key in DERIVED:
            per_matrix = key in ("marginal_std", "loo_std")
            assert got[key].shape == (3,) + (() if per_matrix else lead) + (N,), key
            np.testing.assert_array_equal(got[key], want[key] if per_matrix or lead else want[key][:, 0], err_msg=key)
    assert tuple(model.pointwise_batch(P)) == DERIVED
    assert (len(model.residuals), model._lnprob, model._log_scale, model._glob_snapshot, model._loc_snapshot) == state
    # the formulas on numbers one can check by hand: d = 4, alpha = 6, rhs = 2, diag(C) = 9
    one = SpectrumModel._pointwise_dict(np.full((1, 1), 2.0), np.full((1, 1), 6.0), np.full(1, 4.0), np.full(1, 9.0), True)
    assert {k: float(v[0]) for k, v in one.items()} == dict(alpha=6.0, marginal_std=3.0, loo_mean=0.5, loo_std=0.5, z=3.0,
                                                             log_density=-0.5 * np.log(2.0 * np.pi / 4.0) - 4.5)


def test_shapes_are_checked_and_failures_raise_as_the_likelihood_does():
    model, dev = model_on_a_stand_in(StandIn)
    P = np.tile(model.get_param_vector(), (3, 1))
    for bad in (np.zeros(63), np.zeros((2, 65)), np.zeros((1, 2, 64)), 1.0):
        with pytest.raises(ValueError):
            model.pointwise(bad)
    for bad in (np.zeros(63), np.zeros((2, 2, 64)), np.zeros((3, 2, 63)), np.zeros((1, 3, 2, 64))):
        with pytest.raises(ValueError):
            model.pointwise_batch(P, bad)
    with pytest.raises(ValueError):
        model.pointwise_batch(P[:, :-1])
    assert dev.calls == []
    with pytest.raises(ValueError, match="do not belong"):
        SpectrumModel._pointwise_dict(np.zeros((1, 64)), np.zeros((1, 64)), np.ones(63), np.ones(63), True)
    with pytest.raises(ValueError, match="do not belong"):
        SpectrumModel._pointwise_dict(np.zeros((1, 64)), np.zeros((1, 64)), np.ones(64), np.ones((1, 64)), True)
    dev.info = -1
    with pytest.raises(ValueError, match="outside of original parameter range"):
        model.pointwise()
    dev.info = 7
    with pytest.raises(np.linalg.LinAlgError, match="7-th leading minor"):
        model.pointwise()
    got, info = model.pointwise_batch(P, return_info=True)  # the batch reports instead
    assert (info == 7).all()


# ------------------------------------------------------------------ the contract, in the oracle
def test_alpha_and_the_diagonal_of_the_inverse_give_the_leave_one_out_predictive():
    """Pixel i conditioned on all the others, r_-i: mean C_i,-i C_-i,-i^-1 r_-i and variance C_ii - C_i,-i C_-i,-i^-1 C_-i,i
    (a solve with row and column i deleted) against r_i - alpha_i / d_i and 1 / d_i with alpha = C^-1 r, d = diag(C^-1).
    Both routes are backward-stable solves of systems no worse conditioned than C: N gamma_{3N+1} cond_2(C), relative to the
    leave-one-out standard deviation for the mean and relative for the variance (about 8e-10 here; a wrong formula is off
    by order 1)."""
    N, m = 180, 4
    o = synth.make_order(N=N, m=m, seed=5)
    oo = O.OracleOrder(o["wave"], o["flux"], o["sigma"], o["emu_wl"], o["eigenspectra"], o["flux_mean"], o["flux_std"],
                       o["grid_points"], o["w_hat"])
    p = synth.vector_to_oracle_params(synth.walker_ball(o, B=3, seed=3)[0])
    flux, X, w_cov, _ = O.emulator_terms(oo, p)
    Cj = O.assemble_cov(oo, p, X, w_cov) + 1e-10 * np.eye(N)
    r = flux - oo.flux
    Cinv = np.linalg.inv(Cj)
    alpha, d = np.linalg.solve(Cj, r), np.diag(Cinv)
    tol = N * gamma(3 * N + 1) * np.linalg.cond(Cj)
    worst_mean = worst_var = 0.0
    for i in (0, 1, N // 3, N // 2, N - 2, N - 1):
        keep = np.arange(N) != i
        w = np.linalg.solve(Cj[np.ix_(keep, keep)], Cj[keep, i])
        mean, var = w @ r[keep], Cj[i, i] - w @ Cj[keep, i]
        assert 0 < var < Cj[i, i]
        err_mean = abs((r[i] - alpha[i] / d[i]) - mean) / np.sqrt(var)
        err_var = abs(1.0 / d[i] - var) / var
        worst_mean, worst_var = max(worst_mean, err_mean), max(worst_var, err_var)
        assert err_mean <= tol and err_var <= tol, (i, err_mean, err_var, tol)
    print(f"leave-one-out mean: {worst_mean:.3g} sigma, variance: {worst_var:.3g} relative; tolerance {tol:.3g}; "
          f"diag(C) diag(C^-1) in [{(np.diag(Cj) * d).min():.3g}, {(np.diag(Cj) * d).max():.3g}]")
