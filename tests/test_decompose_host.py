"""The residual decomposition without a device: the refusals of sf_decompose_batch / sf_decompose_workspace_bytes that need
no context (SF_EINVAL and a message before any HIP call; a context needs a device, so what follows the context check is in
tests/test_gpu_decompose.py), the Python-side shape checks and the mapping from the component axis to the keys of
SpectrumModel.residual_components with a stand-in DeviceOrder, and the identity the feature rests on, in the oracle."""
import ctypes as C

import numpy as np
import pytest
from scipy.linalg import cho_factor, cho_solve

from oracle import sf_oracle as O
from starfish_amd import _lib, synth
from starfish_amd.models import SpectrumModel

import stand_in

SF_EINVAL = -1
FAKE = 0x10000  # a non-null "device pointer": a refused call never touches it
U = 2.0 ** -53


def gamma(k):
    return k * U / (1 - k * U)


GOOD = dict(ctx=None, B=4, params=FAKE, rhs=FAKE + (1 << 20), nrhs=3, ldr=4096, rhs_stride=3 * 4096, comp=FAKE + (1 << 24),
            alpha=None, flux=None, info=None, work=FAKE + (1 << 28), work_bytes=1 << 20)

# refused on the counts, the pointers and the right-hand-side conventions: before the context is looked at
BAD = {
    "no walker": dict(B=0),
    "negative batch": dict(B=-3),
    "more walkers than a grid plane": dict(B=65536),
    "no right-hand side": dict(nrhs=0),
    "more right-hand sides than a grid row": dict(nrhs=65536),
    "null params": dict(params=None),
    "null comp": dict(comp=None),
    "negative rhs stride": dict(rhs_stride=-1),
    "the residual as two right-hand sides": dict(rhs=None, nrhs=2),
}


def decompose(lib, md, **kw):
    a = dict(GOOD, **kw)
    return lib.sf_decompose_batch(a["ctx"], md, a["B"], a["params"], a["rhs"], a["nrhs"], a["ldr"], a["rhs_stride"], a["comp"],
                                  a["alpha"], a["flux"], a["info"], a["work"], a["work_bytes"], None)


@pytest.mark.parametrize("case", list(BAD))
def test_decompose_refuses_bad_arguments_before_it_looks_at_the_context(case):
    lib = _lib.load()  # loading needs no GPU; a call that reached the HIP runtime here would not return SF_EINVAL
    rc = decompose(lib, C.byref(_lib.ModelDesc()), **BAD[case])
    assert rc == SF_EINVAL, (case, rc)
    msg = lib.sf_last_error().decode()
    assert msg.startswith("sf_decompose_batch:"), (case, msg)


def test_decompose_entry_points_refuse_a_missing_context_or_model():
    lib = _lib.load()
    md = _lib.ModelDesc()
    for name in ("sf_decompose_workspace_bytes", "sf_decompose_batch", "sf_debug_decompose_matvec"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.sf_decompose_workspace_bytes(None, C.byref(md), 4, 1) == 0
    assert lib.sf_decompose_workspace_bytes(None, C.byref(md), 0, 1) == 0
    assert lib.sf_decompose_workspace_bytes(None, C.byref(md), 4, 0) == 0
    for model in (C.byref(md), None):
        assert decompose(lib, model) == SF_EINVAL
        assert lib.sf_last_error().decode() == "bad context / model descriptor"
        assert decompose(lib, model, rhs=None, nrhs=1, ldr=0, rhs_stride=0) == SF_EINVAL
    assert lib.sf_debug_decompose_matvec(None, C.byref(md), 4, FAKE, 1, FAKE, FAKE, 1 << 20, None) == SF_EINVAL
    assert lib.sf_debug_decompose_matvec(None, C.byref(md), 4, FAKE, 1, None, FAKE, 1 << 20, None) == SF_EINVAL


# ------------------------------------------------------------------ the model methods over a stand-in DeviceOrder
class StandIn(stand_in.StandIn):
    """What SpectrumModel asks of a DeviceOrder here; decompose returns numbers that name their own index."""

    def decompose(self, md, rows, rhs=None, want_flux=False, max_chunk=None):
        B, nrhs = rows.shape[0], 1 if rhs is None else rhs.shape[-2]
        self.calls.append((B, None if rhs is None else rhs.shape))
        b, k, r, i = np.meshgrid(np.arange(B), np.arange(3 + md.n_local), np.arange(nrhs), np.arange(self.n), indexing="ij")
        comp = 1e6 * b + 1e4 * k + 1e3 * r + i
        return dict(comp=comp.astype(float), alpha=-(comp[:, 0] + 0.5), info=np.full(B, self.info, dtype=np.int32))


def model_with(n_local, has_global, N=64):
    def params(o):
        p = dict(synth.centre_params(o))
        p["local_cov"] = [dict(mu=float(o["wave"][5 + 7 * j]), log_amp=-8.0 - j, log_sigma=2.5) for j in range(n_local)]
        if not n_local:
            del p["local_cov"]
        if not has_global:
            del p["global_cov"]
        return p

    return stand_in.model_on_a_stand_in(StandIn, N=N, params=params)


@pytest.mark.parametrize("n_local", [0, 1, 3])
@pytest.mark.parametrize("has_global", [False, True])
def test_component_axis_becomes_the_dict_keys(n_local, has_global):
    model, dev = model_with(n_local, has_global)
    N = 64
    state = (len(model.residuals), model._lnprob, model._log_scale, model._glob_snapshot, model._loc_snapshot)
    keys = ["emulator", "noise"] + ["global"] * has_global + ["local"] * (n_local > 0) + ["alpha"]
    i = np.arange(N)
    for rhs, lead in ((None, ()), (np.zeros(N), ()), (np.zeros((2, N)), (2,))):
        got = model.residual_components(rhs)
        assert list(got) == keys
        r = np.arange(lead[0])[:, None] if lead else 0
        np.testing.assert_array_equal(got["emulator"], 1e3 * r + i)
        np.testing.assert_array_equal(got["noise"], 1e4 + 1e3 * r + i)
        np.testing.assert_array_equal(got["alpha"], -(1e3 * r + i + 0.5))
        if has_global:
            np.testing.assert_array_equal(got["global"], 2e4 + 1e3 * r + i)
        if n_local:
            assert got["local"].shape == (n_local,) + lead + (N,)
            for j in range(n_local):  # in the order of model["local_cov"]
                np.testing.assert_array_equal(got["local"][j], 1e4 * (3 + j) + 1e3 * r + i)
        for key in keys:
            if key != "local":
                assert got[key].shape == lead + (N,)
    assert dev.calls == [(1, None), (1, (1, N)), (1, (2, N))]
    # the batch: the same keys with a leading B axis; row b is the scalar call's entry shifted by the walker's 1e6 b
    P = np.tile(model.get_param_vector(), (3, 1))
    for rhs, lead in ((None, ()), (np.zeros(N), ()), (np.zeros((2, N)), (2,)), (np.zeros((3, 2, N)), (2,))):
        got, info = model.residual_components_batch(P, rhs, return_info=True)
        one = model.residual_components(None if rhs is None else rhs[0] if rhs.ndim == 3 else rhs)
        assert list(got) == keys and info.shape == (3,)
        for key in keys:
            lead_b = (3, n_local) if key == "local" else (3,)
            assert got[key].shape == lead_b + lead + (N,)
            sign = -1 if key == "alpha" else 1
            for b in range(3):
                np.testing.assert_array_equal(got[key][b], one[key] + sign * 1e6 * b)
    assert list(model.residual_components_batch(P)) == keys
    assert (len(model.residuals), model._lnprob, model._log_scale, model._glob_snapshot, model._loc_snapshot) == state


def test_shapes_are_checked_and_failures_raise_as_the_likelihood_does():
    model, dev = model_with(1, True)
    P = np.tile(model.get_param_vector(), (3, 1))
    for bad in (np.zeros(63), np.zeros((2, 65)), np.zeros((1, 2, 64)), 1.0):
        with pytest.raises(ValueError):
            model.residual_components(bad)
    for bad in (np.zeros(63), np.zeros((2, 2, 64)), np.zeros((3, 2, 63)), np.zeros((1, 3, 2, 64))):
        with pytest.raises(ValueError):
            model.residual_components_batch(P, bad)
    with pytest.raises(ValueError):
        model.residual_components_batch(P[:, :-1])
    assert dev.calls == []
    with pytest.raises(ValueError, match="do not belong"):
        SpectrumModel._component_dict(np.zeros((5, 1, 64)), np.zeros((1, 64)), True, 1, True)
    with pytest.raises(ValueError, match="do not belong"):
        SpectrumModel._component_dict(np.zeros((4, 1, 64)), np.zeros((2, 64)), True, 1, True)
    dev.info = -1
    with pytest.raises(ValueError, match="outside of original parameter range"):
        model.residual_components()
    dev.info = 7
    with pytest.raises(np.linalg.LinAlgError, match="7-th leading minor"):
        model.residual_components()
    got, info = model.residual_components_batch(P, return_info=True)  # the batch reports instead
    assert (info == 7).all()


# ------------------------------------------------------------------ the contract, in the oracle
def test_the_conditional_means_of_the_components_add_up_to_the_residual():
    """C = Y^T Y + diag(sigma^2 + 1e-10) + K_global + K_local and alpha = C^-1 r: sum_k K_k alpha = C alpha = r.  Bound:
    the solve's, as tests/test_gpu_apply_factor.py states it for |C alpha - r|, plus the products' (1e-13 + gamma_{n+m+4})
    |C| |alpha| -- the sum identity of tests/test_gpu_decompose.py."""
    N, m = 180, 4
    o = synth.make_order(N=N, m=m, seed=5)
    oo = O.OracleOrder(o["wave"], o["flux"], o["sigma"], o["emu_wl"], o["eigenspectra"], o["flux_mean"], o["flux_std"],
                       o["grid_points"], o["w_hat"])
    p = synth.vector_to_oracle_params(synth.walker_ball(o, B=3, seed=3)[0])
    flux, X, w_cov, _ = O.emulator_terms(oo, p)
    Cj = O.assemble_cov(oo, p, X, w_cov) + 1e-10 * np.eye(N)
    r = flux - oo.flux
    alpha = cho_solve(cho_factor(Cj), r)
    (mu, la, ls), (ga, gl) = p["local_cov"][0], p["global_cov"]
    parts = [X.T @ cho_solve(cho_factor(w_cov), X) @ alpha, (oo.sigma**2 + 1e-10) * alpha,
             O.matern32_global(oo.wave, np.exp(ga), np.exp(gl)) @ alpha, O.gaussian_local(oo.wave, np.exp(la), mu, np.exp(ls)) @ alpha]
    assert all(np.abs(part).max() > 0 for part in parts)
    err = np.abs(np.sum(parts, axis=0) - r).max()
    bound = ((1e-13 + N * gamma(3 * N + 1)) * (np.abs(Cj).sum(axis=1).max() * np.abs(alpha).max() + np.abs(r).max())
             + (1e-13 + gamma(N + m + 4)) * (np.abs(Cj) @ np.abs(alpha)).max())
    print(f"|sum_k K_k alpha - r|_inf = {err:.3g}, bound {bound:.3g}; shares of |r|: "
          + ", ".join(f"{np.abs(part).max() / np.abs(r).max():.3g}" for part in parts))
    assert err <= bound
