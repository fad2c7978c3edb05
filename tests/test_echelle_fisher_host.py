"""Host logic of the multi-order Fisher information: EchelleModel.mean_gradient_labels / _fisher_layout against a brute-force
restatement, reduce_fisher_host against a plain triple loop, the refusals (naming the order), parameter_covariance on a fixed
matrix, and SpectrumModel.parameter_covariance through the shared helper against a copy of the code it replaced.  No device."""
import numpy as np
import pytest

from per_order_cases import PER
from starfish_amd import _device as D
from starfish_amd import _lib, _map, synth
from starfish_amd.models import EchelleModel

import echelle_fisher_cases as EF

NEW_NAMES = ("sf_fisher_banded_multi_workspace_bytes_md", "sf_fisher_banded_multi_batch_md", "sf_multi_fisher_reduce")


class Gauss:
    """A prior with a ``logpdf`` whose second derivative is -1 / s^2 everywhere."""

    def __init__(self, mu, s):
        self.mu, self.s = mu, s

    def logpdf(self, x):
        return -0.5 * ((x - self.mu) / self.s) ** 2


def test_the_new_symbols_are_bound():
    for name in NEW_NAMES:
        assert name in _lib.SIGNATURES


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_labels_and_sources_against_a_brute_force_restatement(name):
    orders, models, em, P = EF.build(name)
    mean = em.mean_gradient_labels
    assert mean == EF.expected_mean_labels(em) and len(mean) == 5 + 3 * 3
    assert not any("global_cov" in k or "local_cov" in k or k.endswith("Rv") for k in mean)
    assert [k for k in em.labels if k in mean] == list(mean)  # labels order
    for solver in ("dense", "banded", "auto", None):
        labels, cols, columns, sources = em._fisher_layout(solver)
        assert labels == em.labels and [len(c) for c in columns] == [8, 8, 8]
        assert sources == EF.expected_sources(em)
        for i, m in enumerate(models):
            assert columns[i] == m._mean_gradient_columns(None, m._model_desc(None))
        for key, src in zip(mean, sources):
            if key.startswith("order"):
                assert len(src) == 1 and src[0][0] == int(key[5])  # an order{i}: label has one source, in its order
            else:
                assert [i for i, _ in src] == [0, 1, 2]  # a shared label has one in every order


def test_rv_has_no_place_in_the_matrix():
    orders = [synth.make_order(N=64, m=2, seed=100 + i, wave0=5000.0 * 1.02**i) for i in range(2)]
    em = EchelleModel.from_orders([synth.build_model(o, params=dict(synth.centre_params(o), Av=0.2, Rv=3.1)) for o in orders])
    assert "Rv" in em.labels and "Av" in em.labels
    assert "Rv" not in em.mean_gradient_labels and "Av" in em.mean_gradient_labels
    assert em._fisher_layout("dense")[3] == EF.expected_sources(em)


def random_units(rng, W, ps):
    out = []
    for p in ps:
        a = rng.standard_normal((W, p, p))
        out.append(a + a.transpose(0, 2, 1))
    return out


def test_reduce_fisher_host_is_the_plain_loop():
    rng = np.random.default_rng(7)
    W, ps = 4, (3, 5, 2)
    fishers = random_units(rng, W, ps)
    lnl = rng.standard_normal((3, W))
    info = np.zeros((3, W), dtype=np.int32)
    info[1, 2] = -2  # a failed unit
    fishers[1][2] = np.nan
    # labels: shared by all three orders; shared by orders 0 and 2; of order 1; of order 0; without a source (an Rv); two more of order 1
    sources = [[(0, 0), (1, 4), (2, 0)], [(0, 2), (2, 1)], [(1, 1)], [(0, 1)], [], [(1, 0)], [(1, 2)]]
    got = D.reduce_fisher_host(lnl, info, fishers, sources)
    want = EF.reduce_restated(lnl, info, fishers, sources)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    total, F, code = got
    assert list(code) == [0, 0, -2, 0] and np.isneginf(total[2]) and np.isnan(F[2]).all()
    good = [0, 1, 3]
    np.testing.assert_array_equal(F[good], F[good].transpose(0, 2, 1))
    # labels of different orders, and the label without a source: exactly 0.0 (not a small number, not -0.0)
    for a, b in ((3, 2), (5, 3), (6, 3), (2, 1), (5, 1)):
        assert (F[good, a, b] == 0.0).all() and not np.signbit(F[good, a, b]).any()
    assert (F[good, 4, :] == 0.0).all() and (F[good, :, 4] == 0.0).all()
    # the sums: label 0 with itself adds all three orders in ascending order, label 0 with label 1 orders 0 and 2
    np.testing.assert_array_equal(F[good, 0, 0], ((fishers[0][:, 0, 0] + fishers[1][:, 4, 4]) + fishers[2][:, 0, 0])[good])
    np.testing.assert_array_equal(F[good, 1, 0], (fishers[0][:, 2, 0] + fishers[2][:, 1, 0])[good])
    np.testing.assert_array_equal(F[good, 5, 2], fishers[1][good, 0, 1])
    with pytest.raises(ValueError, match="two sources"):
        D.reduce_fisher_host(lnl, info, fishers, [[(0, 0), (0, 1)]])


def test_refusals_name_the_order():
    orders, models, em, P = EF.build("A")
    with pytest.raises(ValueError, match="solver must be"):
        em._fisher_layout("sparse")
    models[1].solver = "banded"
    try:
        with pytest.raises(ValueError, match="order 1: .*dense"):
            em._fisher_layout(None)
        assert em._fisher_layout("dense")[3] == EF.expected_sources(em)  # (a named solver does not look at the orders' own)
    finally:
        models[1].solver = "dense"
    # an order with the paper's emulator covariance
    o2 = [synth.make_order(N=64, m=2, seed=100 + i, wave0=5000.0 * 1.02**i) for i in range(2)]
    paper = EchelleModel.from_orders([synth.build_model(o2[0]), synth.build_model(o2[1], emulator_cov="paper")], per_order=PER)
    with pytest.raises(ValueError, match="order 1: .*paper"):
        paper._fisher_layout("banded")
    # more than 16 columns in one order: 5 shared + log_scale + 12 Chebyshev coefficients
    _, many = EF.models_with_cheb((0, 0), [64, 64], 2, (2, 6))
    many[1].params["cheb"] = [0.01, -0.02, 0.004, -0.003, 0.002, -0.001] * 2
    wide = EchelleModel.from_orders(many, per_order=PER)
    assert len(wide.orders[1].mean_gradient_labels) == 18
    with pytest.raises(ValueError, match="order 1: 18 .*at most 16"):
        wide._fisher_layout("banded")
    with pytest.raises(ValueError, match="order 1"):
        wide.fisher_information_batch(wide.get_param_vector()[None, :], solver="banded")


def spd(rng, p):
    a = rng.standard_normal((p, 2 * p))
    scale = 10.0 ** rng.uniform(-2, 2, p)
    return (a @ a.T) * np.outer(scale, scale)


def test_parameter_covariance_on_a_fixed_matrix():
    orders, models, em, P = EF.build("A")
    mean = em.mean_gradient_labels
    p = len(mean)
    F = spd(np.random.default_rng(3), p)
    em.fisher_information = lambda solver=None: F.copy()
    cov = em.parameter_covariance()
    d = np.sqrt(np.diag(F))
    want = np.linalg.inv(F / np.outer(d, d)) / np.outer(d, d)
    np.testing.assert_allclose(cov, want, rtol=1e-9, atol=0)
    assert np.array_equal(cov, cov.T)
    # a prior on a shared label, and a bare per-order key: once per order, on that order's own label
    priors = {"vz": Gauss(10.0, 0.5), "log_scale": Gauss(0.0, 0.1), "global_cov:log_amp": Gauss(-9.0, 1.0)}
    add = np.zeros(p)
    add[mean.index("vz")] = 1 / 0.5**2
    for i in range(3):
        add[mean.index(f"order{i}:log_scale")] = 1 / 0.1**2
    Fp = F + np.diag(add)
    dp = np.sqrt(np.diag(Fp))
    wantp = np.linalg.inv(Fp / np.outer(dp, dp)) / np.outer(dp, dp)
    # (the second difference of a quadratic with step eps^(1/3): rounding of about eps^(1/3) relative to the curvature)
    np.testing.assert_allclose(em.parameter_covariance(priors=priors), wantp, rtol=1e-4, atol=0)
    assert not np.allclose(wantp, want, rtol=1e-3)
    with pytest.raises(ValueError, match="logpdf"):
        em.parameter_covariance(priors={"vz": 3.0})
    em.fisher_information = lambda solver=None: np.ones((p, p))
    with pytest.raises(np.linalg.LinAlgError, match="order0:log_scale.*not positive definite"):
        em.parameter_covariance()
    bad = F.copy()
    bad[2, 2] = -1.0
    em.fisher_information = lambda solver=None: bad
    with pytest.raises(np.linalg.LinAlgError, match="diagonal entry"):
        em.parameter_covariance()


def parameter_covariance_as_it_was(model, F, priors):
    """SpectrumModel.parameter_covariance before the shared helper, with the matrix handed in."""
    priors = model._checked_priors(priors)
    labels = model.mean_gradient_labels
    F = np.array(F, dtype=np.float64)
    for i, key in enumerate(labels):
        if key in priors:
            x = float(model[key])
            h = _map._H0 * max(1.0, abs(x))
            lp = priors[key].logpdf
            F[i, i] -= (lp(x + h) - 2.0 * lp(x) + lp(x - h)) / (h * h)
    d = np.sqrt(np.diag(F))
    L = np.linalg.cholesky(F / np.outer(d, d))
    Li = np.linalg.solve(L, np.eye(len(labels)))
    return (Li.T @ Li) / np.outer(d, d)


def test_spectrum_model_parameter_covariance_keeps_its_bits():
    model = synth.build_model(synth.make_order(N=64, m=2, seed=5))
    p = len(model.mean_gradient_labels)
    F = spd(np.random.default_rng(11), p)
    model.fisher_information = lambda solver=None: F.copy()
    for priors in (None, {"vz": Gauss(10.0, 0.5), "cheb:2": Gauss(0.0, 0.01), "global_cov:log_amp": Gauss(-9.0, 1.0)}):
        np.testing.assert_array_equal(model.parameter_covariance(priors=priors), parameter_covariance_as_it_was(model, F, priors))
    model.fisher_information = lambda solver=None: np.ones((p, p))
    with pytest.raises(np.linalg.LinAlgError, match="not positive definite"):
        model.parameter_covariance()
