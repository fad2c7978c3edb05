"""The Fisher information of the mean-flux parameters without a device: the new C-ABI names, what the calls refuse before they
look at a context (the slot checks that need one -- a repeated column, a covariance column -- are in tests/test_gpu_fisher.py),
the numpy helper of the GPU test (tests/fisher_reference.py) column by column against Richardson differences of its own flux,
its Woodbury form against its dense form, the teeth of the entry bound, and the host logic of SpectrumModel.parameter_covariance
and samplers.gaussian_ball over a stand-in DeviceOrder."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from scipy import stats

from starfish_amd import _lib, samplers, synth
from starfish_amd.models import SpectrumModel

import fisher_reference as FR
import mean_derivatives as MD
from gpu_helpers import oracle_order
from stand_in import StandIn as HostStandIn, model_on_a_stand_in, state_of
from test_mean_gradient_host import MEAN, STEPS, richardson

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
NEW_NAMES = {"sf_fisher_mean_workspace_bytes": 4, "sf_fisher_mean_batch": 13, "sf_fisher_banded_mean_workspace_bytes": 5,
             "sf_fisher_banded_mean_batch": 15, "sf_fisher_banded_max_slots": 2}
EINVAL, FAKE = -1, 0x10000  # (a pointer that is not NULL; the calls below return before they read it)
LD = np.longdouble


def test_new_entry_points_are_declared_bound_and_exported():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "starfish_amd.h")).read()
    for name, nargs in NEW_NAMES.items():
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        declared = re.search(rf"\b{name}\s*\(([^;]*)\);", header)
        assert declared and declared.group(1).count(",") + 1 == nargs, name
    assert callable(getattr(samplers, "gaussian_ball", None))
    for name in ("fisher_information", "fisher_information_batch", "parameter_covariance"):
        assert callable(getattr(SpectrumModel, name, None)), name


# ------------------------------------------------------------------------------------------ refusals
def model_desc():
    md = _lib.ModelDesc()
    md.has_log_scale = md.has_vz = md.has_vsini = 1
    return md


def dense_rc(lib, slots=(2, 1), nslots=None, stride=None, params=FAKE, lnl=FAKE, fisher=FAKE, work=FAKE):
    nslots = len(slots) if nslots is None else nslots
    h_slots = (C.c_int * max(len(slots), 1))(*slots) if slots is not None else None
    stride = nslots * nslots if stride is None else stride
    return lib.sf_fisher_mean_batch(None, C.byref(model_desc()), 3, params, h_slots, nslots, lnl, fisher, stride, None, work, 1 << 40,
                                    None)


def banded_rc(lib, halfwidth=100, slots=(2, 1), nslots=None, stride=None, params=FAKE, lnl=FAKE, fisher=FAKE, work=FAKE):
    nslots = len(slots) if nslots is None else nslots
    h_slots = (C.c_int * max(len(slots), 1))(*slots) if slots is not None else None
    stride = nslots * nslots if stride is None else stride
    return lib.sf_fisher_banded_mean_batch(None, C.byref(model_desc()), 3, params, halfwidth, h_slots, nslots, lnl, fisher, stride,
                                           None, None, work, 1 << 40, None)


BAD = [(dict(params=None), "required"), (dict(lnl=None), "required"), (dict(fisher=None), "required"), (dict(work=None), "required"),
       (dict(slots=None, nslots=2), "required"), (dict(slots=(), nslots=0), "nslots=0"), (dict(slots=tuple(range(17))), "nslots=17"),
       (dict(stride=3), "fisher_stride=3")]


@pytest.mark.parametrize("call,name", [(dense_rc, "sf_fisher_mean_batch"), (banded_rc, "sf_fisher_banded_mean_batch")])
def test_fisher_calls_refuse_before_they_look_at_the_context(call, name):
    lib = _lib.load()
    for kw, word in BAD:
        assert call(lib, **kw) == EINVAL, kw
        msg = lib.sf_last_error().decode()
        assert msg.startswith(name + ":") and word in msg, (kw, msg)
    assert call(lib) == EINVAL  # (no context)
    assert lib.sf_last_error().decode() == "bad context / model descriptor"


def test_banded_call_refuses_a_half_width_past_the_window_naming_the_dense_call():
    lib = _lib.load()
    # the window's limits at the row count the slots alone imply (no context: at least one low-rank row): 144 up to 16 rows, ...
    for kw in (dict(halfwidth=-1), dict(halfwidth=145), dict(halfwidth=160), dict(halfwidth=129, slots=tuple(range(15))),
               dict(halfwidth=800)):
        assert banded_rc(lib, **kw) == EINVAL, kw
        msg = lib.sf_last_error().decode()
        assert "sf_fisher_mean_batch" in msg and "window" in msg, (kw, msg)
    assert banded_rc(lib, halfwidth=144) == EINVAL and lib.sf_last_error().decode() == "bad context / model descriptor"


def test_workspace_queries_return_zero_for_what_the_calls_refuse():
    lib = _lib.load()
    md = model_desc()
    for nslots in (0, 2, 17):
        assert lib.sf_fisher_mean_workspace_bytes(None, C.byref(md), 3, nslots) == 0
        assert lib.sf_fisher_banded_mean_workspace_bytes(None, C.byref(md), 3, 100, nslots) == 0
    assert lib.sf_fisher_mean_workspace_bytes(None, None, 3, 2) == 0
    assert lib.sf_fisher_banded_mean_workspace_bytes(None, None, 3, 100, 2) == 0
    assert lib.sf_fisher_banded_mean_workspace_bytes(None, C.byref(md), 3, 160, 2) == 0
    assert lib.sf_fisher_banded_max_slots(None, 100) == EINVAL


# ------------------------------------------------------------------------------------------ the helper
_REFS = {}


def walker(N, m, b=0):
    """(oracle order, parameters of walker b, fisher_reference.reference of them): made once, never written."""
    if (N, m, b) not in _REFS:
        o = synth.make_order(N=N, m=m, seed=5)
        oo = oracle_order(o)
        vec = synth.walker_ball(o, B=3, seed=3)[b]
        p = synth.vector_to_oracle_params(vec)
        _REFS[N, m, b] = (oo, vec, p, FR.reference(oo, p, MEAN))
    return _REFS[N, m, b]


def test_every_helper_column_agrees_with_richardson_differences_of_the_helpers_own_flux():
    """The criterion of tests/test_mean_gradient_host.py: with d(h) the central difference quotient and R = (4 d(h/2) - d(h)) / 3
    the column lies within 4 |d(h) - d(h/2)| of R, plus the rounding of the flux over the step."""
    oo, vec, p, ref = walker(180, 4)
    for j, name in enumerate(MEAN):
        i = synth.LABELS.index(name)

        def flux(x):
            v = vec.copy()
            v[i] = x
            return MD.tangents(oo, synth.vector_to_oracle_params(v))[0]

        R, spread = richardson(flux, vec[i], STEPS[name])
        tol = 4 * spread.max() + 1e-13 * np.abs(flux(vec[i])).max() / STEPS[name]
        err = np.abs(ref["J"][:, j] - R).max()
        print(f"{name}: max |column| {np.abs(ref['J'][:, j]).max():.3g}, max |column - R| {err:.3g}, allowed {tol:.3g}")
        assert err <= tol, (name, err, tol)


@pytest.mark.parametrize("N,m", [(180, 4), (330, 4), (180, 17)])
def test_woodbury_form_agrees_with_the_dense_form(N, m):
    """Both in float64 against the longdouble dense form, normalised by sqrt(F_ii F_jj).  Measured: Woodbury 4.6e-16 (N180),
    6.0e-16 (N330), 7.2e-16 (N180 m17); dense 8.8e-16, 9.8e-16, 1.2e-15.  The margin is 8 x the 9e-16 of the issue's CPU check.
    G_JJ,ii / F_ii is at most 1.007 (measured 1.003, 1.006, 1.006): the difference G_JJ - U^T U does not cancel."""
    oo, vec, p, ref = walker(N, m)
    F = ref["Fld"].astype(np.float64)
    d = np.sqrt(np.diag(F))
    wood = (np.abs(ref["Fw"] - F) / np.outer(d, d)).max()
    dense = (np.abs(ref["F64"] - F) / np.outer(d, d)).max()
    ratio = (np.diag(ref["GJJ"]) / np.diag(F)).max()
    print(f"N{N} m{m}: |Woodbury - longdouble| {wood:.3g}, |dense float64 - longdouble| {dense:.3g} of sqrt(F_ii F_jj); "
          f"max G_JJ,ii / F_ii {ratio:.4f}; smallest eigenvalue of D^-1 F D^-1 {np.linalg.eigvalsh(FR.normalised(F))[0]:.3g}")
    assert wood <= 8 * 9e-16 and dense <= 8 * 9e-16
    assert ratio <= 1.01
    assert np.array_equal(ref["F64"], ref["F64"].T)


def wrong_weights(oo, p, ref):
    """F with a wrong weight, three ways: the factor 2 of the cheb / Av slots dropped, U^T U omitted, jitter left out."""
    flux = MD.tangents(oo, p)[0]
    J = ref["J"].copy()
    x = oo.wave / oo.wave.max()
    for k in (1, 2):  # T_k (A' + M') in place of T_k (2 A' + M'): T_k f / p
        J[:, MEAN.index(f"cheb:{k}")] = np.polynomial.chebyshev.chebval(x, [0] * k + [1]) * flux / MD.cheb_series(oo, p)
    _, X, S = FR.jacobian(oo, p, MEAN)
    return {"factor 2 dropped": FR.fisher_dense(J, ref["C"]),
            "U^T U omitted": FR.fisher_woodbury(ref["J"], ref["Bd"], ref["Y"], drop_uu=True)[0],
            "no jitter": FR.fisher_dense(ref["J"], FR.covariance(oo, p, X, S, jitter=False))}


@pytest.mark.parametrize("N,m", [(180, 4), (180, 17)])
def test_the_entry_bound_has_teeth(N, m):
    oo, vec, p, ref = walker(N, m)
    F = ref["Fld"].astype(np.float64)
    for banded in (False, True):
        bound, terms = FR.entry_bound(ref, banded=banded)
        inside = max((np.abs(ref["F64"] - F) / bound).max(), (np.abs(ref["Fw"] - F) / bound).max())
        print(f"N{N} m{m} banded={banded}: float64 helper at {inside:.3g} of the bound; largest term / sqrt(F_ii F_jj): "
              + ", ".join(f"{k} {(v / np.sqrt(np.outer(np.diag(F), np.diag(F)))).max():.3g}" for k, v in terms.items()))
        assert inside <= 1.0
        for name, wrong in wrong_weights(oo, p, ref).items():
            outside = (np.abs(wrong - F) / bound).max()
            print(f"    {name}: {outside:.3g} of the bound")
            assert outside > 10.0, (name, outside)


# ------------------------------------------------------------------------------------------ the model's host logic
class StandIn(HostStandIn):
    """fisher_mean names its columns: F = A^T A + diag(1 + column) of a fixed well-conditioned A, per walker b scaled by 1 + b."""
    singular = False

    def fisher_mean(self, md, rows, slots, solver="dense", max_chunk=None):
        B, p = rows.shape[0], len(slots)
        self.calls.append(("fisher", B, tuple(slots), solver))
        A = np.random.default_rng(7).standard_normal((p + 3, p))
        F = A.T @ A + np.diag(1.0 + np.asarray(slots, dtype=np.float64))
        if self.singular:
            F[:, 1] = F[:, 0]
            F[1, :] = F[0, :]
        return dict(lnl=-100.0 - np.arange(B), fisher=F[None] * (1.0 + np.arange(B))[:, None, None],
                    info=np.full(B, self.info, dtype=np.int32))


def test_fisher_information_follows_the_thawed_labels_and_parameter_covariance_inverts_it():
    model, dev = model_on_a_stand_in(StandIn, freeze=("global_cov", "local_cov"))
    labels = model.mean_gradient_labels
    assert labels == MEAN
    column = {"vsini": 0, "vz": 1, "log_scale": 2, "T": 6, "logg": 7, "Z": 8, "cheb:1": 9, "cheb:2": 10}
    state = state_of(model)
    F = model.fisher_information()
    assert dev.calls[-1] == ("fisher", 1, tuple(column[k] for k in labels), "dense") and F.shape == (8, 8)
    Fb, info = model.fisher_information_batch(np.tile(model.get_param_vector(), (3, 1)), return_info=True, solver="auto")
    assert dev.calls[-1][1:] == (3, tuple(column[k] for k in labels), "auto") and (info == 0).all()
    np.testing.assert_array_equal(Fb[0], F)
    np.testing.assert_array_equal(Fb[2], 3 * F)
    cov = model.parameter_covariance()
    assert np.abs(cov @ F - np.eye(8)).max() <= 1e-12 and np.array_equal(cov, cov.T)
    # a normal prior adds 1 / sigma^2 on its label's diagonal entry, to within the second difference's error: h^2 / 12 f''''
    # vanishes for a quadratic, what remains is the rounding 4 eps |logpdf| / h^2 (h = eps^(1/3) max(1, |x|) ~ 6e-6 |x|)
    sigma = 0.05
    x = float(model["logg"])
    prior = stats.norm(x + 0.01, sigma)
    with_prior = model.parameter_covariance(priors={"logg": prior})
    Fp = F.copy()
    j = labels.index("logg")
    Fp[j, j] += 1 / sigma**2
    h = np.finfo(np.float64).eps ** (1 / 3) * max(1.0, abs(x))
    slack = 4 * np.finfo(np.float64).eps * abs(prior.logpdf(x)) / h**2
    got = np.linalg.inv(with_prior)
    print(f"prior on logg: added {got[j, j] - F[j, j]!r}, 1 / sigma^2 = {1 / sigma**2!r}, allowed error {slack:.3g}")
    assert abs(got[j, j] - Fp[j, j]) <= slack + 1e-9 * Fp[j, j]
    assert np.abs(with_prior @ Fp - np.eye(8)).max() <= 1e-6
    assert with_prior[j, j] < cov[j, j]
    assert state_of(model) == state
    model.freeze(["vsini", "T", "cheb:1"])
    kept = tuple(k for k in MEAN if k not in ("vsini", "T", "cheb:1"))
    assert model.parameter_covariance(solver="banded").shape == (5, 5)
    assert dev.calls[-1] == ("fisher", 1, tuple(column[k] for k in kept), "banded")


def test_a_singular_fisher_matrix_raises_naming_the_labels():
    model, dev = model_on_a_stand_in(StandIn, freeze=("global_cov", "local_cov"))
    dev.singular = True
    with pytest.raises(np.linalg.LinAlgError, match="vz.*vsini.*not positive definite"):
        model.parameter_covariance()


def test_models_the_device_does_not_differentiate_are_refused():
    model, dev = model_on_a_stand_in(StandIn, emulator_cov="paper")
    with pytest.raises(ValueError, match="paper"):
        model.fisher_information()
    o = synth.make_order(N=64, m=3, seed=9)
    params = synth.centre_params(o)
    del params["log_scale"]
    model = synth.build_model(o, params=params)
    model._device = lambda: StandIn(64)
    with pytest.raises(ValueError, match="log_scale"):
        model.fisher_information_batch(model.get_param_vector()[None, :])
    model, dev = model_on_a_stand_in(StandIn)
    with pytest.raises(ValueError, match="solver"):
        model.fisher_information(solver="sparse")
    with pytest.raises(ValueError, match="Invalid priors"):
        model.parameter_covariance(priors={"nope": stats.norm(0, 1)})
    model.freeze([k for k in model.labels if not k.startswith("local_cov")])
    with pytest.raises(ValueError, match="no thawed mean-flux parameter"):
        model.parameter_covariance()
    assert dev.calls == []
    model, dev = model_on_a_stand_in(StandIn, freeze=("global_cov", "local_cov"))
    dev.info = -1
    with pytest.raises(ValueError, match="outside of original parameter range"):
        model.fisher_information()


def test_gaussian_ball_has_the_shape_and_the_covariance_asked_for():
    rng = np.random.default_rng(11)
    A = rng.standard_normal((6, 4))
    scale = np.array([1e-3, 1.0, 50.0, 2.0])
    cov = (A.T @ A) * np.outer(scale, scale)
    x = np.array([5.0, -1.0, 6000.0, 0.0])
    n = 40000
    ball = samplers.gaussian_ball(x, cov, n, seed=3)
    assert ball.shape == (n, 4)
    np.testing.assert_array_equal(ball, samplers.gaussian_ball(x, cov, n, seed=3))
    # sampling error: the mean within 5 sigma / sqrt(n); a sample covariance entry has variance (C_ii C_jj + C_ij^2) / (n - 1)
    d = np.sqrt(np.diag(cov))
    assert (np.abs(ball.mean(axis=0) - x) <= 5 * d / np.sqrt(n)).all()
    se = np.sqrt((np.outer(d, d) ** 2 + cov**2) / (n - 1))
    z = np.abs(np.cov(ball.T) - cov) / se
    print("gaussian_ball: largest |sample cov - cov| / standard error", z.max())
    assert z.max() <= 5.0
    assert samplers.gaussian_ball(x, cov, 8).shape == (8, 4)
    with pytest.raises(np.linalg.LinAlgError):
        samplers.gaussian_ball(x[:2], np.array([[1.0, 2.0], [2.0, 1.0]]), 4)
    with pytest.raises(ValueError):
        samplers.gaussian_ball(x, cov[:3, :3], 4)
