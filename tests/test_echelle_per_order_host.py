"""Host-only: the parameter book-keeping of an EchelleModel with per-order nuisance parameters (label layout, vector
and dict round trips, freeze / thaw routing, prior terms, refusals).  No device work: the models are never evaluated."""
import numpy as np
import pytest

from starfish_amd import Spectrum, synth
from starfish_amd.models import EchelleModel

from per_order_cases import PER, SHARED, expected_labels, per_order_models


class Flat:
    """A prior whose value names the parameter value it saw (so a sum of terms can be checked)."""

    def __init__(self, scale=1.0):
        self.scale = scale

    def logpdf(self, x):
        return self.scale * np.asarray(x, dtype=np.float64)


class Never:
    def logpdf(self, x):
        return -np.inf * np.ones_like(np.asarray(x, dtype=np.float64))


def test_label_layout_shared_first_then_each_order():
    _, models = per_order_models()
    em = EchelleModel.from_orders(models, per_order=list(PER))
    labels = em.labels
    assert labels == expected_labels(models)
    assert labels[: len(SHARED)] == SHARED
    assert "order0:cheb:2" in labels and "order2:local_cov:2:log_sigma" in labels
    assert not any(k.startswith("order0:local_cov") for k in labels)  # order 0 has no local kernel
    assert sum(k.startswith("order1:local_cov") for k in labels) == 3
    assert sum(k.startswith("order2:local_cov") for k in labels) == 9
    # the vector holds the orders' own values
    vec = em.get_param_vector()
    d = dict(zip(labels, vec))
    assert d["order1:cheb:1"] == pytest.approx(0.02) and d["order2:log_scale"] == pytest.approx(0.2)
    assert d["vz"] == models[0]["vz"]


def test_per_order_none_keeps_the_shared_layout():
    orders = synth.make_echelle(3, N=64, m=2)
    models = [synth.build_model(o, freeze=("local_cov",)) for o in orders]
    em = EchelleModel.from_orders(models)
    assert em.per_order is None and em.labels == synth.SHARED_LABELS
    models[1].thaw("local_cov")
    with pytest.raises(ValueError):
        EchelleModel.from_orders(models)


def test_vector_round_trip_routes_shared_and_prefixed_values():
    _, models = per_order_models()
    em = EchelleModel.from_orders(models, per_order=PER)
    labels = em.labels
    P = np.arange(1.0, len(labels) + 1.0)
    em.set_param_vector(P)
    np.testing.assert_array_equal(em.get_param_vector(), P)
    for i, m in enumerate(models):
        own = dict(zip(m.labels, m.get_param_vector()))
        for k in SHARED:
            assert own[k] == P[labels.index(k)]  # shared values go to every order
        for k, v in own.items():
            if k.split(":")[0] in PER:
                assert v == P[labels.index(f"order{i}:{k}")]
    with pytest.raises(ValueError):
        em.set_param_vector(P[:-1])


def test_dict_round_trip_flat_and_nested():
    _, models = per_order_models()
    em = EchelleModel.from_orders(models, per_order=PER)
    flat = em.get_param_dict(flat=True)
    assert tuple(flat.keys()) == em.labels
    np.testing.assert_array_equal(np.array(list(flat.values())), em.get_param_vector())
    nested = em.get_param_dict()
    assert nested["order2"]["cheb"]["1"] == pytest.approx(0.03)
    assert nested["vz"] == models[0]["vz"]
    em.set_param_dict({"order1:cheb:2": 0.5, "vz": 3.0, "order2": {"log_scale": -0.7}})
    assert models[1]["cheb"] == [pytest.approx(0.02), 0.5]
    assert models[0]["cheb"][1] == models[2]["cheb"][1] == -0.02
    assert all(m["vz"] == 3.0 for m in models)
    assert models[2]["log_scale"] == -0.7 and models[1]["log_scale"] == pytest.approx(0.1)
    # a bare per-order key goes to every order that has it
    em.set_param_dict({"local_cov:0:log_amp": -7.5})
    assert models[1]["local_cov:0:log_amp"] == models[2]["local_cov:0:log_amp"] == -7.5
    assert "local_cov" not in models[0].params
    with pytest.raises(KeyError):
        em.set_param_dict({"nonsense": 1.0})


def test_freeze_thaw_prefixed_acts_on_one_order_bare_on_all():
    _, models = per_order_models()
    em = EchelleModel.from_orders(models, per_order=PER)
    n0 = len(em.labels)
    em.freeze("order1:cheb:2")
    assert "order1:cheb:2" not in em.labels and "order0:cheb:2" in em.labels and len(em.labels) == n0 - 1
    em.freeze("order2:local_cov")
    assert not any(k.startswith("order2:local_cov") for k in em.labels)
    assert sum(k.startswith("order1:local_cov") for k in em.labels) == 3
    em.thaw("order2:local_cov")
    assert sum(k.startswith("order2:local_cov") for k in em.labels) == 9
    # bare names: every order (an order without the group is left alone)
    em.freeze("local_cov")
    assert not any(":local_cov" in k for k in em.labels)
    assert "local_cov" not in models[0].frozen
    em.thaw(["local_cov", "order1:cheb:2"])
    assert len(em.labels) == n0
    em.freeze("vz")  # a shared parameter: frozen in every order, the layout stays consistent
    assert "vz" not in em.labels and all("vz" in m.frozen for m in models)
    em.thaw("vz")
    with pytest.raises(ValueError):
        em.freeze("order1:vz")  # vz is shared in this model
    with pytest.raises(ValueError):
        em.freeze("order7:cheb:1")  # no such order
    em.freeze("all")
    assert em.labels == ()
    em.thaw("all")
    assert len(em.labels) == n0


def test_priors_bare_key_per_order_shared_key_once():
    _, models = per_order_models()
    em = EchelleModel.from_orders(models, per_order=PER)
    labels = em.labels
    P = np.tile(em.get_param_vector(), (3, 1))
    P[:, labels.index("order0:log_scale")] = [1.0, 2.0, 3.0]
    P[:, labels.index("vz")] = [10.0, 20.0, 30.0]
    cols = em._layout()[1]
    # bare per-order key: one term per order; shared key once
    lp = em._batch_prior(P, {"log_scale": Flat(), "vz": Flat(100.0)}, cols)
    np.testing.assert_allclose(lp, P[:, labels.index("order0:log_scale")] + 0.1 + 0.2 + 100.0 * P[:, labels.index("vz")])
    # prefixed key: that order only; a bare key of a group member only counts orders that have it
    lp = em._batch_prior(P, {"order2:log_scale": Flat(), "local_cov:2:log_amp": Flat()}, cols)
    np.testing.assert_allclose(lp, 0.2 + models[2]["local_cov:2:log_amp"])
    lp = em._batch_prior(P, {"local_cov:0:log_amp": Flat()}, cols)
    np.testing.assert_allclose(lp, models[1]["local_cov:0:log_amp"] + models[2]["local_cov:0:log_amp"])
    # a frozen parameter's prior uses its current value
    em.freeze("order1:log_scale")
    labels, cols = em._layout()
    lp = em._batch_prior(P[:, [i for i, k in enumerate(expected_labels(models)) if k != "order1:log_scale"]],
                        {"order1:log_scale": Flat()}, cols)
    np.testing.assert_allclose(lp, 0.1)
    # a non-finite prior is -inf before any device work (the models have never been evaluated)
    assert em.log_likelihood({"order2:log_scale": Never()}) == -np.inf
    assert all(m._dev is None for m in models)


def test_batch_rejects_a_vector_of_the_wrong_length():
    _, models = per_order_models()
    em = EchelleModel.from_orders(models, per_order=PER)
    with pytest.raises(ValueError):
        em.log_likelihood_batch(np.zeros((2, len(em.labels) + 1)))
    # every walker's prior is -inf: no device work, all -inf
    lnl, info = em.log_likelihood_batch(np.tile(em.get_param_vector(), (2, 1)), priors={"vz": Never()}, return_info=True)
    assert (lnl == -np.inf).all() and (info == 0).all()
    assert all(m._dev is None for m in models)


def test_refusals():
    orders, models = per_order_models()
    with pytest.raises(ValueError, match="grid parameter"):
        EchelleModel.from_orders(models, per_order=["cheb", "T"])
    with pytest.raises(ValueError):
        EchelleModel.from_orders(models, per_order=["Rv"])
    models[1].freeze("vz")  # the shared labels now disagree
    with pytest.raises(ValueError, match="shared"):
        EchelleModel.from_orders(models, per_order=PER)


def test_constructor_takes_per_order_as_a_keyword():
    orders = synth.make_echelle(2, N=64, m=2)
    emu_models = [synth.build_model(o) for o in orders]
    emu = emu_models[0].emulator
    wave = np.stack([orders[0]["wave"], orders[0]["wave"] * 1.001])
    flux = np.stack([orders[0]["flux"], orders[0]["flux"]])
    data = Spectrum(wave, flux, sigmas=np.full_like(flux, 0.01))
    c = dict(synth.centre_params(orders[0]))
    gp = c.pop("grid_params")
    em = EchelleModel(emu, data, gp, per_order=["cheb", "log_scale"], **c)
    assert em.per_order == ("cheb", "log_scale")
    assert all("per_order" not in m.params for m in em.orders)
    shared = tuple(k for k in synth.LABELS if not k.startswith(("cheb", "log_scale")))
    assert em.labels == shared + ("order0:log_scale", "order0:cheb:1", "order0:cheb:2",
                                  "order1:log_scale", "order1:cheb:1", "order1:cheb:2")
    assert em.get_param_dict(flat=True)["order1:cheb:2"] == -0.02
    with pytest.raises(ValueError):
        EchelleModel(emu, data, gp, per_order=["logg"], **c)
    plain = EchelleModel(emu, data, gp, **c)
    assert plain.per_order is None and plain.labels == synth.LABELS


def test_cut_units_keeps_unit_order_and_never_exceeds_the_cap():
    """The cut of a multi-order unit list into calls (starfish_amd._multi.cut_units): pieces of ``(order, lo, hi)``."""
    from starfish_amd._multi import cut_units

    assert cut_units([3, 3, 3], 4) == [[(0, 0, 3), (1, 0, 1)], [(1, 1, 3), (2, 0, 2)], [(2, 2, 3)]]
    for sizes in ([3, 3, 3], [1], [5, 1, 7, 2], [64, 130, 180, 96]):
        total = sum(sizes)
        units = [(i, u) for i, n in enumerate(sizes) for u in range(n)]
        for cap in (total, total + 9):  # cap >= total: one piece of whole orders
            assert cut_units(sizes, cap) == [[(i, 0, n) for i, n in enumerate(sizes)]]
        assert cut_units(sizes, 1) == [[(i, u, u + 1)] for i, u in units]  # cap = 1: one unit per piece
        for cap in range(1, total + 1):
            pieces = cut_units(sizes, cap)
            assert [(i, u) for piece in pieces for i, lo, hi in piece for u in range(lo, hi)] == units  # each once, in order
            counts = [sum(hi - lo for _, lo, hi in piece) for piece in pieces]
            assert max(counts) <= cap and all(c == cap for c in counts[:-1]) and all(hi > lo for p in pieces for _, lo, hi in p)
