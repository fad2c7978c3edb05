"""The Python layer's single statements -- starfish_amd._rows (the C-ABI parameter row) and starfish_amd._map (the L-BFGS-B
MAP search) -- against numbers written out here, on the CPU: the row of four descriptors at P = 3, the rows SpectrumModel._pack
builds, the prior's central difference, and the trainer differences the other host tests do not cover."""
import numpy as np
import pytest

from starfish_amd import _device as D
from starfish_amd import _map
from starfish_amd import _rows as R

import stand_in
from stand_in import model_on_a_stand_in, state_of

GRID = {"T": 6, "logg": 7, "Z": 8}
FIXED = {"vsini": 0, "vz": 1, "log_scale": 2}


def kernels(o, n):
    return [dict(mu=float(o["wave"][5 + 7 * j]), log_amp=-8.0 - j, log_sigma=2.5) for j in range(n)]


def local_labels(first, n):
    return {f"local_cov:{i}:{leaf}": first + 3 * i + j for i in range(n) for j, leaf in enumerate(("mu", "log_amp", "log_sigma"))}


# (descriptor arguments, model parameters beyond vz / vsini / log_scale / grid, stride, columns of the labels beyond FIXED and
# GRID, slices grid / cheb / local, av, covariance-gradient slots of the labels)
CASES = {
    "bare": (dict(has_global=0, n_local=0, n_cheb=0, has_av=0), lambda o: {}, 9, {}, (6, 9), (9, 9), (9, 9), None, {}),
    "global_1local_2cheb": (
        dict(has_global=1, n_local=1, n_cheb=2, has_av=0),
        lambda o: dict(global_cov=dict(log_amp=-9.0, log_ls=2.0), local_cov=kernels(o, 1), cheb=[0.01, -0.02]), 14,
        {"global_cov:log_amp": 4, "global_cov:log_ls": 5, "cheb:1": 9, "cheb:2": 10, **local_labels(11, 1)},
        (6, 9), (9, 11), (11, 14), None,
        {"global_cov:log_amp": 0, "global_cov:log_ls": 1, "local_cov:0:mu": 2, "local_cov:0:log_amp": 3, "local_cov:0:log_sigma": 4}),
    "global_3local_4cheb_av": (
        dict(has_global=1, n_local=3, n_cheb=4, has_av=1),
        lambda o: dict(global_cov=dict(log_amp=-9.0, log_ls=2.0), local_cov=kernels(o, 3), cheb=[0.01, -0.02, 0.03, 0.04],
                       Av=0.2, Rv=3.1), 23,
        {"global_cov:log_amp": 4, "global_cov:log_ls": 5, "cheb:1": 9, "cheb:2": 10, "cheb:3": 11, "cheb:4": 12,
         **local_labels(13, 3), "Av": 22, "Rv": None},
        (6, 9), (9, 13), (13, 22), 22,
        {"global_cov:log_amp": 0, "global_cov:log_ls": 1, **local_labels(2, 3)}),
    "2local": (dict(has_global=0, n_local=2, n_cheb=0, has_av=0), lambda o: dict(local_cov=kernels(o, 2)), 15,
               local_labels(9, 2), (6, 9), (9, 9), (9, 15), None, local_labels(0, 2)),
}


def model_of(case, cls=stand_in.StandIn):
    extra = CASES[case][1]
    return model_on_a_stand_in(cls, params=lambda o: dict(vz=10.0, vsini=30.0, log_scale=0.0, grid_params=[6050.0, 4.2, -0.3],
                                                          **extra(o)))


def explicit_rows(model, P):
    """The rows of ``P`` (labels order) by explicit indexing, as tests/gpu_helpers.pack_rows writes them; frozen parameters
    from the model's store."""
    x = dict(model.params.items())
    rows = np.zeros((len(P), 6 + 3 + sum(k.startswith("cheb:") for k in x) + sum(k.startswith("local_cov:") for k in x)
                     + ("Av" in x)))
    for r, p in zip(rows, P):
        v = dict(x, **dict(zip(model.labels, p)))
        r[0], r[1], r[2], r[3] = v["vsini"], v["vz"], v["log_scale"], 1.0
        if "global_cov:log_amp" in v:
            r[4], r[5] = v["global_cov:log_amp"], v["global_cov:log_ls"]
        r[6:9] = v["T"], v["logg"], v["Z"]
        nc = sum(k.startswith("cheb:") for k in v)
        r[9 : 9 + nc] = [v[f"cheb:{c}"] for c in range(1, nc + 1)]
        nl = sum(k.startswith("local_cov:") for k in v) // 3
        for k in range(nl):
            r[9 + nc + 3 * k : 9 + nc + 3 * k + 3] = [v[f"local_cov:{k}:{leaf}"] for leaf in ("mu", "log_amp", "log_sigma")]
        if "Av" in v:
            r[9 + nc + 3 * nl] = v["Av"]
    return rows


@pytest.mark.parametrize("case", list(CASES))
def test_the_row_layout_of_four_descriptors_at_three_grid_parameters(case):
    desc, _, stride, columns, grid, cheb, local, av, cov_slots = CASES[case]
    md = R.model_desc(1, 1, 1, **desc)
    assert D.model_desc_key(md) == (1, 1, 1, desc["has_global"], desc["n_local"], desc["n_cheb"], 0, desc["has_av"])
    assert D.model_desc_key(D.DeviceOrder.model_desc(None, 1, 1, 1, **desc)) == D.model_desc_key(md)
    assert (R.VSINI, R.VZ, R.LOG_SCALE, R.NORM, R.GLOBAL_LOG_AMP, R.GLOBAL_LOG_LS) == (0, 1, 2, 3, 4, 5)
    assert (R.GLOBAL.start, R.GLOBAL.stop) == (4, 6)
    lay = R.RowLayout(3, md)
    assert [(s.start, s.stop) for s in (lay.grid, lay.cheb, lay.local)] == [grid, cheb, local] and lay.av == av
    assert [(lay.local_of(i).start, lay.local_of(i).stop) for i in range(desc["n_local"])] == \
        [(local[0] + 3 * i, local[0] + 3 * i + 3) for i in range(desc["n_local"])]
    assert R.cov_grad_slots(md) == len(cov_slots) == 2 * desc["has_global"] + 3 * desc["n_local"]
    assert {key: R.cov_grad_slot(md, key) for key in cov_slots} == cov_slots
    # the model's own view of the same row: every label's column, on the stand-in and without a device
    model, dev = model_of(case)
    assert D.model_desc_key(model._model_desc(dev)) == D.model_desc_key(md) == D.model_desc_key(model._model_desc(None))
    assert dev.param_stride(md) == stride
    want = {**FIXED, **GRID, **columns}
    assert set(model.labels) == set(want)
    for slots in (model._slot_of(dev, md), model._slot_of(None, md)):
        assert {key: slots.get(key) for key in model.labels} == want
    assert model.gradient_labels == tuple(cov_slots) and model._gradient_slots(md) == list(cov_slots.values())
    assert model._mean_gradient_columns(dev, md) == [want[k] for k in model.labels if k not in cov_slots and k != "Rv"]


@pytest.mark.parametrize("case", list(CASES))
def test_pack_builds_the_rows_that_explicit_indexing_builds(case):
    model, dev = model_of(case)
    stride = CASES[case][2]
    x0 = model.get_param_vector()
    P = x0 + np.random.default_rng(3).uniform(-0.1, 0.1, (3, len(x0)))
    _, md, rows = model._pack(P, update_caches=False)
    assert rows.shape == (3, stride)
    np.testing.assert_array_equal(rows, explicit_rows(model, P))
    np.testing.assert_array_equal(model._pack(None, update_caches=False)[2], explicit_rows(model, x0[None, :]))
    hw = D.band_halfwidth_bound(model.data.wave, rows, 3, bool(md.has_global), md.n_local, md.n_cheb)
    assert hw.shape == (3,) and ((hw > 0) == bool(md.has_global or md.n_local)).all()


def test_pack_keeps_a_frozen_groups_snapshot_and_asks_the_emulator_for_the_norm():
    model, dev = model_of("global_3local_4cheb_av")
    for group in ("global_cov", "local_cov"):
        model.freeze(group)
    assert model._glob_snapshot is None and model._loc_snapshot is None
    seen = explicit_rows(model, model.get_param_vector()[None, :])[0]
    model._pack()  # (fills the snapshots of the frozen groups)
    assert model._glob_snapshot == tuple(seen[4:6]) and np.array_equal(np.ravel(model._loc_snapshot), seen[13:22])
    model.params["global_cov:log_amp"] = -5.0  # the store moves on; the frozen groups keep what their caches saw
    model.params["local_cov:1:mu"] = 1.0
    P = model.get_param_vector() + np.random.default_rng(4).uniform(-0.1, 0.1, (3, len(model.labels)))
    want = explicit_rows(model, P)
    assert (want[:, 4] == -5.0).all() and (want[:, 16] == 1.0).all()
    want[:, 4:6], want[:, 13:22] = seen[4:6], seen[13:22]
    np.testing.assert_array_equal(model._pack(P, update_caches=False)[2], want)
    grids = []
    model.norm = True
    model.emulator.norm_factor = lambda g: grids.append(np.array(g)) or 2.0 + np.atleast_2d(g)[:, 0]
    want[:, 3] = 2.0 + want[:, 6]
    np.testing.assert_array_equal(model._pack(P, update_caches=False)[2], want)
    np.testing.assert_array_equal(grids[0], want[:, 6:9])


# ------------------------------------------------------------------ _map: the prior's value and slope
class Gaussian:
    """log N(x; mu, s^2) and its slope in closed form."""

    def __init__(self, mu, s):
        self.mu, self.s, self.c = mu, s, np.log(s * np.sqrt(2 * np.pi))

    def logpdf(self, x):
        z = (x - self.mu) / self.s
        return -(z * z) / 2 - self.c

    def slope(self, x):
        return -(x - self.mu) / self.s**2


@pytest.mark.parametrize("x", [0.0, 1e-3, 1e6])
def test_prior_slope_is_the_central_difference_and_within_its_own_error_of_the_closed_form(x):
    """The central difference (f(x + h) - f(x - h)) / (2 h) misses f'(x) by its truncation error h^2 / 6 |f'''|, the next
    term of the Taylor series (zero here: a Gaussian's logpdf is a quadratic), plus its rounding error: each of the two
    values is known to about eps |f| / 2, so their difference over 2 h to eps |f| / h."""
    prior = Gaussian(0.3, 2.0)
    eps = np.finfo(np.float64).eps
    h = eps ** (1.0 / 3.0) * max(1.0, abs(x))
    value, slope = _map.prior_value_and_slope(prior, x)
    assert value == prior.logpdf(x)
    assert slope == (prior.logpdf(x + h) - prior.logpdf(x - h)) / (2 * h)
    third_derivative = 0.0
    bound = h * h / 6 * abs(third_derivative) + eps * abs(prior.logpdf(x)) / h
    err = abs(slope - prior.slope(x))
    print(f"x = {x:g}: h = {h:.3g}, slope {slope:.17g}, closed form {prior.slope(x):.17g}, error {err:.3g}, bound {bound:.3g}")
    assert err <= bound


# ------------------------------------------------------------------ the trainer differences no other host test holds
class Bowl(stand_in.StandIn):
    """Both gradient calls of a concave bowl around 1 in the columns they differentiate in; every call notes the state the
    model was in."""
    model = None

    def _bowl(self, rows, x):
        self.calls.append(state_of(self.model))
        return dict(lnl=-100.0 - 0.5 * ((x - 1) ** 2).sum(axis=1), grad=-(x - 1), info=np.full(len(rows), self.info, np.int32))

    def loglike_grad(self, md, rows, want_flux=False, max_chunk=None):
        return self._bowl(rows, rows[:, [4, 5, 11, 12, 13]])  # (the centre model: global, two Chebyshev terms, one local)

    def loglike_mean_grad(self, md, rows, slots, want_flux=False, max_chunk=None):
        return self._bowl(rows, rows[:, list(slots)])


def test_train_covariance_leaves_the_model_alone_until_it_succeeds_and_only_then():
    model, dev = model_on_a_stand_in(Bowl)
    dev.model = model
    start = state_of(model)
    soln = model.train_covariance(options=dict(maxiter=1))
    assert soln.status == 1 and not soln.success and not np.allclose(soln.x, 1.0)  # the iteration limit: best point so far
    assert len(dev.calls) > 1 and all(state == start for state in dev.calls)
    assert state_of(model) == start  # ... which train_covariance, unlike train(gradient=True), does not adopt
    dev.calls.clear()
    soln = model.train_covariance()
    assert soln.success and all(state == start for state in dev.calls)
    np.testing.assert_allclose(soln.x, 1.0, atol=1e-5)
    np.testing.assert_array_equal([model[k] for k in model.gradient_labels], soln.x)
    cov = [model.labels.index(k) for k in model.gradient_labels]
    assert np.delete(model.get_param_vector(), cov).tolist() == np.delete(np.array(start[5]), cov).tolist()


def test_train_gradient_forces_jac_and_adopts_the_point_of_an_iteration_limit():
    model, dev = model_on_a_stand_in(Bowl, freeze=("global_cov", "local_cov"))
    dev.model = model
    soln = model.train(gradient=True, jac=False)  # (scipy would take the (value, slope) pair for the value)
    assert soln.success
    np.testing.assert_allclose(soln.x, 1.0, atol=1e-5)
    model, dev = model_on_a_stand_in(Bowl, freeze=("global_cov", "local_cov"))
    dev.model = model
    soln = model.train(gradient=True, options=dict(maxiter=1))
    assert soln.status == 1 and not soln.success
    np.testing.assert_array_equal(model.get_param_vector(), soln.x)
    # every evaluation found the model at its own point: the states differ from call to call
    assert len({state[5] for state in dev.calls}) == len(dev.calls) > 1
