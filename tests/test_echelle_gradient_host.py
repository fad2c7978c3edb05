"""Host logic of EchelleModel's gradient (no device): the label -> (order, slot) column map, the refusals, the new C-ABI
names and the prior handling of train()."""
import re

import numpy as np
import pytest

from per_order_cases import PER, per_order_models
from starfish_amd import _device as D
from starfish_amd import _lib, synth
from starfish_amd.models import EchelleModel, SpectrumModel

import echelle_gradient_cases as EG

NEW_NAMES = {"sf_multi_grad_workspace_bytes_md": 5, "sf_loglike_multi_grad_batch_md": 12, "sf_multi_grad_reduce": 14}


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    def refuse(self):
        raise AssertionError("the host logic asked for a device")

    monkeypatch.setattr(SpectrumModel, "_device", refuse)


def per_order_model(n_local=(0, 1, 3), sizes=(64, 130, 180)):
    _, models = per_order_models(n_local, sizes=list(sizes), m=2, seed0=100)
    return models, EchelleModel.from_orders(models, per_order=PER)


def test_new_entry_points_are_declared_bound_and_exported():
    lib = _lib.load()
    header = open(_lib.os.path.join(_lib._HERE, "..", "include", "starfish_amd.h")).read()
    for name, nargs in NEW_NAMES.items():
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        assert re.search(rf"\b{name}\s*\(", header), name
    assert "sf_grad_request" in header
    assert [f for f, _ in _lib.GradRequest._fields_] == ["h_mean_slots", "n_mean_slots", "want_cov"]
    assert _lib.C.sizeof(_lib.GradRequest) == 16
    for name in ("MultiGradPlan", "loglike_multi_grad", "reduce_orders_host", "column_map_csr"):
        assert hasattr(D, name), name
    for name in ("log_likelihood_gradient_batch", "log_likelihood_gradient", "train"):
        assert callable(getattr(EchelleModel, name)), name


def test_column_map_of_per_order_models_with_different_numbers_of_local_kernels():
    models, em = per_order_model()
    labels, cols, requests, sources = em._gradient_layout()
    assert labels == em.labels and len(labels) == 32
    assert sources == EG.expected_sources(em)
    for key in ("vz", "vsini", "T", "logg", "Z"):
        j = labels.index(key)
        assert [i for i, _ in sources[j]] == [0, 1, 2]  # a shared label: every order, ascending
    assert sources[labels.index("order2:local_cov:2:log_sigma")] == [(2, 8 + 2 + 3 * 2 + 2)]
    assert sources[labels.index("order0:global_cov:log_ls")] == [(0, 8 + 1)]
    # every order asks for its eight mean columns (vz, vsini, log_scale, cheb:1, cheb:2, T, logg, Z) and its kernels
    for (columns, want_cov), m in zip(requests, models):
        assert want_cov and columns == [1, 0, 2, 9, 10, 6, 7, 8]
    for i, c in enumerate(cols):
        assert [labels[j].split(":", 1)[1] if labels[j].startswith("order") else labels[j] for j in c] == list(models[i].labels)


def test_column_map_after_freezing_and_with_rv():
    models, em = per_order_model()
    em.freeze(["vz", "order1:cheb:1", "order2:local_cov:0:mu", "order0:global_cov"])
    labels, cols, requests, sources = em._gradient_layout()
    assert "vz" not in labels and "order1:cheb:1" not in labels and not any(k.startswith("order0:global_cov") for k in labels)
    assert sources == EG.expected_sources(em)
    assert requests[0] == ([0, 2, 9, 10, 6, 7, 8], False)  # order 0 has no local kernel and its global one is frozen
    assert requests[1] == ([0, 2, 10, 6, 7, 8], True)
    # a unit's row holds ALL covariance slots of its descriptor: a frozen mu does not move the others
    assert sources[labels.index("order2:local_cov:0:log_amp")] == [(2, 7 + 2 + 1)]
    csr_ptr, csr_src = D.column_map_csr(sources)
    assert csr_ptr.dtype == np.int32 and csr_src.dtype == np.int32 and csr_src.shape == (csr_ptr[-1], 2)
    assert list(np.diff(csr_ptr)) == [len(s) for s in sources]


def test_column_map_of_shared_models():
    orders = synth.make_echelle(3, 64)
    em = synth.build_echelle(orders)
    assert em.per_order is None
    labels, cols, requests, sources = em._gradient_layout()
    assert labels == tuple(em.orders[0].labels)
    assert sources == EG.expected_sources(em)
    assert all([i for i, _ in src] == [0, 1, 2] for src in sources)
    assert all(len({slot for _, slot in src}) == 1 for src in sources)


def test_refusals_name_the_order_and_need_no_device():
    models, em = per_order_model()
    models[1].solver = "auto"
    with pytest.raises(ValueError, match=r"order 1: .*dense"):
        em.log_likelihood_gradient_batch(np.zeros((1, 32)))
    with pytest.raises(ValueError, match=r"order 1: .*dense"):
        em.train()
    models[1].solver = "dense"
    models[2].emulator_cov = "paper"
    with pytest.raises(ValueError, match=r'order 2: .*emulator_cov="paper"'):
        em.log_likelihood_gradient()
    models[2].emulator_cov = "code"
    models[0].norm = True
    with pytest.raises(ValueError, match=r"order 0: norm=True with a thawed grid parameter"):
        em.log_likelihood_gradient_batch(np.zeros((1, 32)))
    models[0].norm = False
    em._gradient_layout()  # (every refusal above is gone again)
    # an order without log_scale whose mean labels are thawed
    _, others = per_order_models((0, 1), sizes=[64, 64], m=2, seed0=100)
    del others[1]["log_scale"]
    em2 = EchelleModel.from_orders(others, per_order=PER)
    with pytest.raises(ValueError, match=r"order 1: the mean gradient needs log_scale"):
        em2.log_likelihood_gradient_batch(np.zeros((1, len(em2.labels))))
    # ... which is fine once only its covariance labels are left
    others[1].freeze([k for k in others[1].labels if not k.startswith(("global_cov", "local_cov"))])
    with pytest.raises(ValueError, match="shared thawed parameters"):
        em2._gradient_layout()  # (the shared labels now disagree: the model's own check)
    em.freeze("all")
    with pytest.raises(ValueError, match="no thawed parameter"):
        em.log_likelihood_gradient_batch(np.zeros((1, 0)))
    with pytest.raises(ValueError, match="no thawed parameter"):
        em.train()


def test_plan_refuses_an_empty_request_before_any_device_work():
    with pytest.raises(ValueError, match="nothing to differentiate"):
        D.MultiGradPlan([None], [D.DeviceOrder.model_desc(None, 1, 1, 1, 1, 0, 2)], [np.zeros((1, 11))], [([], False)])
    with pytest.raises(ValueError, match="2 requests for 1 orders"):
        D.MultiGradPlan([None], [None], [None], [([], True)] * 2)


def test_reduce_orders_host_follows_the_rule_of_the_device_kernel():
    rng = np.random.default_rng(3)
    lnl, info = rng.standard_normal((3, 5)) * 1e3, np.zeros((3, 5), dtype=np.int32)
    info[1, 2], info[2, 2], info[0, 4] = 7, -1, -2
    grads = [rng.standard_normal((5, k)) for k in (4, 2, 6)]
    sources = [[(0, 1), (1, 0), (2, 5)], [], [(2, 0)], [(1, 1), (0, 3)]]
    got = D.reduce_orders_host(lnl, info, grads, sources)
    want = EG.reduce_restated(lnl, info, grads, [sorted(s) for s in sources])
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
    assert list(got[2]) == [0, 0, 7, 0, -2] and np.isneginf(got[0][[2, 4]]).all() and np.isnan(got[1][[2, 4]]).all()
    assert (got[1][[0, 1, 3], 1] == 0.0).all()


def test_train_adds_priors_and_their_slopes_and_converges_on_a_quadratic(monkeypatch):
    """The device call replaced by lnL = -1/2 |x - a|^2: with a normal prior N(c, s) on a label the optimum of that label is
    (a + c / s^2) / (1 + 1 / s^2).  A bare per-order key counts once per order, a prefixed key for its order, a shared key once;
    a prior on a frozen parameter is a constant."""
    from scipy.stats import norm

    models, em = per_order_model()
    em.freeze("order1:global_cov:log_ls")
    labels = em.labels
    rng = np.random.default_rng(0)
    x0 = em.get_param_vector()
    a = x0 + 0.3 * rng.standard_normal(len(labels))
    calls = []

    def fake(P, return_info=False, return_orders=False):
        P = np.atleast_2d(P)
        calls.append(P.copy())
        return -0.5 * np.sum((P - a) ** 2, axis=1), -(P - a), np.zeros(len(P), dtype=np.int32)

    monkeypatch.setattr(em, "log_likelihood_gradient_batch", fake)
    priors = {"log_scale": norm(0.2, 0.5), "order2:cheb:1": norm(0.0, 0.1), "T": norm(x0[labels.index("T")] + 5.0, 10.0),
              "order1:global_cov:log_ls": norm(2.0, 1.0)}
    want = a.copy()
    hit = {f"order{i}:log_scale": (0.2, 0.5) for i in range(3)}
    hit.update({"order2:cheb:1": (0.0, 0.1), "T": (x0[labels.index("T")] + 5.0, 10.0)})
    for key, (c, s) in hit.items():
        j = labels.index(key)
        want[j] = (a[j] + c / s**2) / (1 + 1 / s**2)
    soln = em.train(priors=priors, options=dict(maxiter=200, ftol=1e-15, gtol=1e-10))
    assert soln.success, soln.message
    np.testing.assert_allclose(soln.x, want, rtol=0, atol=2e-6)
    np.testing.assert_array_equal(em.get_param_vector(), soln.x)
    const = norm(2.0, 1.0).logpdf(models[1]["global_cov:log_ls"])
    value = -0.5 * np.sum((soln.x - a) ** 2) + const + sum(norm(c, s).logpdf(soln.x[labels.index(k)]) for k, (c, s) in hit.items())
    assert abs(-soln.fun - value) <= 1e-12 * max(1.0, abs(value))
    assert all(p.shape == (1, len(labels)) for p in calls)
    with pytest.raises(ValueError, match="logpdf"):
        em.train(priors={"T": 3.0})


def test_train_raises_for_a_point_the_device_flags(monkeypatch):
    models, em = per_order_model()
    n = len(em.labels)
    monkeypatch.setattr(em, "log_likelihood_gradient_batch",
                        lambda P, return_info=False, return_orders=False: (np.array([-np.inf]), np.full((1, n), np.nan),
                                                                           np.array([-1], dtype=np.int32)))
    with pytest.raises(ValueError, match="outside of original parameter range"):
        em.train()
    with pytest.raises(ValueError, match="outside of original parameter range"):
        em.log_likelihood_gradient()
