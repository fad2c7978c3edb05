"""The Fisher information of the covariance hyper-parameters without a device: the new C-ABI names, what sf_fisher_cov_batch
refuses before it looks at a context, the numpy helper of the GPU test (tests/cov_fisher_reference.py) against a route that uses
no derivative formula, and the host logic of SpectrumModel.covariance_fisher_information / parameter_covariance(
include_covariance=True) and samplers.gaussian_ball over a stand-in DeviceOrder."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from scipy import stats

from oracle import sf_oracle as O
from starfish_amd import _lib, _map, samplers, synth
from starfish_amd.models import SpectrumModel

import cov_derivatives as CD
import cov_fisher_reference as CF
from gpu_helpers import oracle_order
from stand_in import StandIn as HostStandIn, model_on_a_stand_in, state_of

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
NEW_NAMES = {"sf_fisher_cov_workspace_bytes": 3, "sf_fisher_cov_batch": 11, "sf_debug_fisher_cov_contract": 9}
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
    for name in ("covariance_fisher_information", "covariance_fisher_information_batch", "parameter_covariance"):
        assert callable(getattr(SpectrumModel, name, None)), name
    assert isinstance(getattr(SpectrumModel, "fisher_labels", None), property)


# ------------------------------------------------------------------------------------------ refusals
def model_desc(has_global=1, n_local=1):
    md = _lib.ModelDesc()
    md.has_global, md.n_local = has_global, n_local
    return md


GOOD = dict(md=(1, 1), B=3, params=FAKE, lnl=None, fisher=FAKE, stride=25, info=None)
BAD = [(dict(B=0), "B=0"), (dict(B=-2), "B=-2"), (dict(B=65536), "B=65536"), (dict(params=None), "required"),
       (dict(fisher=None), "required"), (dict(md=(0, 0)), "nothing to differentiate"), (dict(stride=24), "fisher_stride=24"),
       (dict(md=(0, 2), stride=35), "fisher_stride=35")]


def fisher_cov_rc(lib, **kw):
    a = dict(GOOD, **kw)
    return lib.sf_fisher_cov_batch(None, C.byref(model_desc(*a["md"])), a["B"], a["params"], a["lnl"], a["fisher"], a["stride"],
                                   a["info"], FAKE, 1 << 40, None)


@pytest.mark.parametrize("kw,word", BAD)
def test_fisher_cov_refuses_before_it_looks_at_the_context(kw, word):
    lib = _lib.load()
    assert fisher_cov_rc(lib, **kw) == EINVAL, kw
    msg = lib.sf_last_error().decode()
    assert msg.startswith("sf_fisher_cov_batch:") and word in msg, (kw, msg)
    a = dict(GOOD, **kw)
    assert lib.sf_fisher_cov_workspace_bytes(None, C.byref(model_desc(*a["md"])), a["B"]) == 0


def test_with_good_counts_the_missing_context_is_what_is_refused():
    lib = _lib.load()
    assert fisher_cov_rc(lib) == EINVAL  # (d_lnl and d_info may be NULL)
    assert lib.sf_last_error().decode() == "bad context / model descriptor"
    assert lib.sf_fisher_cov_workspace_bytes(None, C.byref(model_desc()), 3) == 0
    assert lib.sf_fisher_cov_workspace_bytes(None, None, 3) == 0
    rc = lib.sf_debug_fisher_cov_contract(None, C.byref(model_desc()), 3, FAKE, FAKE, 24, FAKE, 1 << 40, None)
    assert rc == EINVAL and lib.sf_last_error().decode().startswith("sf_debug_fisher_cov_contract:")


# ------------------------------------------------------------------------------------------ the helper
def two_local_params(o, vec):
    """The parameters of case N180-two-local of tests/test_gpu_gradient.py, restated."""
    p = synth.vector_to_oracle_params(vec)
    w = o["wave"]
    n = len(w)
    del p["global_cov"]
    (mu, la, ls), = p["local_cov"]
    p["local_cov"] = [(mu, la, ls), (float(w[n - 10] + 0.37 * (w[n - 9] - w[n - 10])), la - 0.3, ls + 0.02)]
    return p


def with_slot(p, label, value):
    """A copy of the oracle parameter dict with the covariance slot ``label`` set to ``value``."""
    q = dict(p)
    parts = label.split(":")
    if parts[0] == "global_cov":
        g = list(p["global_cov"])
        g[CD.GLOBAL_SLOTS.index(parts[1])] = value
        q["global_cov"] = tuple(g)
    else:
        loc = [list(t) for t in p["local_cov"]]
        loc[int(parts[1])][CD.LOCAL_SLOTS.index(parts[2])] = value
        q["local_cov"] = [tuple(t) for t in loc]
    return q


def slot_value(p, label):
    parts = label.split(":")
    if parts[0] == "global_cov":
        return p["global_cov"][CD.GLOBAL_SLOTS.index(parts[1])]
    return p["local_cov"][int(parts[1])][CD.LOCAL_SLOTS.index(parts[2])]


@pytest.mark.parametrize("name", ["N180", "N180-two-local"])
def test_the_helper_is_minus_the_hessian_of_the_expected_likelihood(name):
    """-F is the Hessian at theta0 of lbar(theta) = -1/2 tr(C(theta)^-1 C(theta0)) - 1/2 logdet C(theta): the expectation of the
    likelihood over data drawn at theta0.  lbar comes from the oracle's matrices alone (longdouble Cholesky of the float64
    matrix); its Hessian by central second differences with steps 2e-2 and 1e-2 and one Richardson step, (4 H(h/2) - H(h)) / 3.
    Every pair of slots that are not a mu (lbar has kinks in mu), walker 0.  Agreement to 1e-6 sqrt(F_ii F_jj); measured on the
    CPU when the bound was set: worst 3.9e-8 (N180) and 2.5e-8 (N180-two-local); with this file's lbar in longdouble 3.0e-8 and
    2.4e-8 (what remains is the truncation of the difference quotient)."""
    N = 180
    o = synth.make_order(N=N, m=4, seed=5)
    oo = oracle_order(o)
    vec = synth.walker_ball(o, B=3, seed=3)[0]
    p0 = two_local_params(o, vec) if name.endswith("two-local") else synth.vector_to_oracle_params(vec)
    jitter = O.JITTER * np.eye(N)
    C0 = O.forward_model(oo, p0)[1] + jitter
    named = CD.slot_derivatives(o["wave"], p0, dtype=LD)
    F = CF.fisher_cov(C0, [d for _, d in named]).astype(np.float64)
    keep = [i for i, (label, _) in enumerate(named) if not label.endswith(":mu")]
    assert len(keep) == 4
    C0l = C0.astype(LD)

    cache = {}

    def lbar(shifts):
        key = tuple(sorted(shifts.items()))
        if key not in cache:
            p = p0
            for label, dx in shifts.items():
                p = with_slot(p, label, slot_value(p0, label) + dx)
            Lc = CF.cholesky_longdouble((O.forward_model(oo, p)[1] + jitter).astype(LD))
            X = CF.inverse_longdouble(Lc)
            cache[key] = -LD(0.5) * np.sum((X.T @ X) * C0l) - np.sum(np.log(np.diag(Lc)))
        return cache[key]

    def hessian(a, b, h):
        if a == b:
            return (lbar({a: h}) - 2 * lbar({}) + lbar({a: -h})) / (h * h)
        return (lbar({a: h, b: h}) - lbar({a: h, b: -h}) - lbar({a: -h, b: h}) + lbar({a: -h, b: -h})) / (4 * h * h)

    worst = 0.0
    for x, i in enumerate(keep):
        for j in keep[:x + 1]:
            a, b = named[i][0], named[j][0]
            H = (4 * hessian(a, b, 1e-2) - hessian(a, b, 2e-2)) / 3
            ratio = abs(float(-H) - F[i, j]) / np.sqrt(F[i, i] * F[j, j])
            worst = max(worst, ratio)
            print(f"{name} ({a}, {b}): F = {F[i, j]:.10g}, -Hessian = {float(-H):.10g}, |difference| / sqrt(F_ii F_jj) = {ratio:.3g}")
            assert ratio <= 1e-6, (a, b, F[i, j], float(-H))
    print(f"{name}: worst ratio {worst:.3g}")
    # the float64 form of the helper and its size
    F64 = CF.fisher_cov(C0, [d.astype(np.float64) for _, d in named], np.float64)
    size = CF.size(CF.cinv(C0, np.float64), [d for _, d in CD.slot_derivatives(o["wave"], p0, absolute=True)])
    assert (np.abs(F64 - F) <= 1e-6 * size).all() and (np.abs(F) <= size * (1 + 1e-12)).all()
    assert np.array_equal(F64, F64.T) or np.abs(F64 - F64.T).max() <= 1e-12 * np.abs(F64).max()


# ------------------------------------------------------------------------------------------ the model's host logic
class StandIn(HostStandIn):
    """fisher_cov and fisher_mean return well-conditioned matrices that name their slots; walker b scaled by 1 + b."""
    singular = False

    @staticmethod
    def _matrix(seed, marks):
        p = len(marks)
        A = np.random.default_rng(seed).standard_normal((p + 3, p))
        return A.T @ A + np.diag(1.0 + np.asarray(marks, dtype=np.float64))

    def fisher_cov(self, md, rows, max_chunk=None):
        B, s = rows.shape[0], (2 if md.has_global else 0) + 3 * md.n_local
        self.calls.append(("fisher_cov", B, s))
        F = self._matrix(5, range(s))
        if self.singular:
            F[:, 1] = F[:, 0]
            F[1, :] = F[0, :]
        return dict(lnl=-100.0 - np.arange(B), fisher=F[None] * (1.0 + np.arange(B))[:, None, None],
                    info=np.full(B, self.info, dtype=np.int32))

    def fisher_mean(self, md, rows, slots, solver="dense", max_chunk=None):
        B = rows.shape[0]
        self.calls.append(("fisher", B, tuple(slots), solver))
        return dict(lnl=-100.0 - np.arange(B), fisher=self._matrix(7, slots)[None] * (1.0 + np.arange(B))[:, None, None],
                    info=np.full(B, self.info, dtype=np.int32))


def two_local(o):
    params = synth.centre_params(o)
    params["local_cov"] = params["local_cov"] + [dict(mu=float(o["wave"][40]), log_amp=-8.5, log_sigma=2.5)]
    return params


def test_covariance_fisher_information_follows_the_thawed_labels():
    model, dev = model_on_a_stand_in(StandIn, params=two_local)
    assert len(model.gradient_labels) == 8
    raw = StandIn._matrix(5, range(8))
    state = state_of(model)
    F = model.covariance_fisher_information()
    assert dev.calls[-1] == ("fisher_cov", 1, 8)
    np.testing.assert_array_equal(F, raw)
    Fb, info = model.covariance_fisher_information_batch(np.tile(model.get_param_vector(), (3, 1)), return_info=True)
    assert Fb.shape == (3, 8, 8) and (info == 0).all()
    np.testing.assert_array_equal(Fb[2], 3 * raw)
    assert state_of(model) == state
    model.freeze(["local_cov:0:mu", "global_cov:log_ls", "vz"])
    kept = [0, 3, 4, 5, 6, 7]
    assert len(model.gradient_labels) == 6
    np.testing.assert_array_equal(model.covariance_fisher_information(), raw[np.ix_(kept, kept)])
    Fb = model.covariance_fisher_information_batch(np.tile(model.get_param_vector(), (2, 1)))
    np.testing.assert_array_equal(Fb[1], 2 * raw[np.ix_(kept, kept)])
    assert all(call[2] == 8 for call in dev.calls)  # (the device differentiates in every slot)
    model.freeze("local_cov")
    np.testing.assert_array_equal(model.covariance_fisher_information(), raw[:1, :1])


def test_fisher_labels_and_the_block_diagonal_assembly():
    model, dev = model_on_a_stand_in(StandIn)
    labels = model.labels
    assert model.fisher_labels == tuple(labels) and "Rv" not in labels
    mean = [labels.index(k) for k in model.mean_gradient_labels]
    cov = [labels.index(k) for k in model.gradient_labels]
    assert sorted(mean + cov) == list(range(len(labels))) and min(cov) > min(mean) and max(cov) < max(mean)
    state = state_of(model)
    default = model.parameter_covariance()
    np.testing.assert_array_equal(default, _map.laplace_covariance(model.fisher_information(), model.mean_gradient_labels, []))
    assert not any(call[0] == "fisher_cov" for call in dev.calls)
    F = np.zeros((len(labels), len(labels)))
    F[np.ix_(mean, mean)] = model.fisher_information()
    F[np.ix_(cov, cov)] = model.covariance_fisher_information()
    full = model.parameter_covariance(include_covariance=True)
    np.testing.assert_array_equal(full, _map.laplace_covariance(F, labels, []))
    assert full.shape == (len(labels),) * 2 and np.array_equal(full, full.T)
    assert (full[np.ix_(mean, cov)] == 0).all()
    np.testing.assert_allclose(full[np.ix_(mean, mean)], default, rtol=1e-10, atol=0)
    assert np.abs(full @ F - np.eye(len(labels))).max() <= 1e-10
    # priors on either kind of label
    pri = {"logg": stats.norm(float(model["logg"]), 0.05), "global_cov:log_amp": stats.norm(float(model["global_cov:log_amp"]), 0.5)}
    with_pri = model.parameter_covariance(priors=pri, include_covariance=True)
    terms = [(labels.index(k), pri[k], float(model[k])) for k in labels if k in pri]
    np.testing.assert_array_equal(with_pri, _map.laplace_covariance(F, labels, terms))
    for k in pri:
        i = labels.index(k)
        assert with_pri[i, i] < full[i, i]
    assert state_of(model) == state
    # either block may be empty
    model.freeze(["global_cov", "local_cov"])
    np.testing.assert_array_equal(model.parameter_covariance(include_covariance=True), model.parameter_covariance())
    model.thaw(["global_cov", "local_cov"])
    model.freeze([k for k in model.labels if not k.startswith(("global_cov", "local_cov"))])
    only = model.parameter_covariance(include_covariance=True)
    np.testing.assert_array_equal(only, _map.laplace_covariance(model.covariance_fisher_information(), model.gradient_labels, []))
    with pytest.raises(ValueError, match="no thawed mean-flux parameter"):
        model.parameter_covariance()


def test_nothing_thawed_is_a_value_error_and_failures_raise_as_the_likelihood_does():
    model, dev = model_on_a_stand_in(StandIn)
    dev.info = -1
    with pytest.raises(ValueError, match="outside of original parameter range"):
        model.covariance_fisher_information()
    dev.info = 7
    with pytest.raises(np.linalg.LinAlgError, match="7-th leading minor"):
        model.covariance_fisher_information()
    F, info = model.covariance_fisher_information_batch(np.tile(model.get_param_vector(), (2, 1)), return_info=True)
    assert (info == 7).all()
    dev.info = 0
    model.freeze(["global_cov", "local_cov"])
    calls = len(dev.calls)
    for call in (model.covariance_fisher_information, lambda: model.covariance_fisher_information_batch(np.zeros((2, len(model.labels))))):
        with pytest.raises(ValueError, match="no thawed global_cov / local_cov"):
            call()
    assert len(dev.calls) == calls
    model.freeze(list(model.labels))
    with pytest.raises(ValueError):
        model.parameter_covariance(include_covariance=True)


def test_a_singular_covariance_block_raises_naming_the_labels():
    model, dev = model_on_a_stand_in(StandIn)
    dev.singular = True
    with pytest.raises(np.linalg.LinAlgError, match="global_cov:log_amp.*global_cov:log_ls.*not positive definite"):
        model.parameter_covariance(include_covariance=True)


def test_gaussian_ball_over_the_fisher_labels_has_the_shape_and_covariance_asked_for():
    model, dev = model_on_a_stand_in(StandIn)
    cov = model.parameter_covariance(include_covariance=True)
    labels = model.fisher_labels
    x = np.array([float(model[k]) for k in labels])
    np.testing.assert_array_equal(x, model.get_param_vector())
    n = 40000
    ball = samplers.gaussian_ball(x, cov, n, seed=3)
    assert ball.shape == (n, len(labels))
    d = np.sqrt(np.diag(cov))
    assert (np.abs(ball.mean(axis=0) - x) <= 5 * d / np.sqrt(n)).all()
    se = np.sqrt((np.outer(d, d) ** 2 + cov**2) / (n - 1))
    z = np.abs(np.cov(ball.T) - cov) / se
    print("gaussian_ball over fisher_labels: largest |sample cov - cov| / standard error", z.max())
    assert z.max() <= 5.0
