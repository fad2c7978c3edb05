"""SpectrumModel.residual_components / residual_components_batch on the device: keys and shapes, the DeviceOrder result
behind them, alpha = cho_solve() bit for bit, the sum of the components, and that the model's state is left alone."""
import numpy as np
import pytest

from starfish_amd import synth

pytestmark = pytest.mark.gpu

N = 180
_MODEL = {}


def shared():
    """The model (one global, one local kernel), its scalar result and the DeviceOrder call behind it (made once)."""
    if not _MODEL:
        o = synth.make_order(N=N, m=4, seed=5)
        model = synth.build_model(o)
        dev, md, rows = model._pack(update_caches=False)
        _MODEL.update(o=o, model=model, dec=dev.decompose(md, rows, want_flux=True), got=model.residual_components())
    return _MODEL


def test_keys_shapes_and_the_device_result():
    s = shared()
    got, dec = s["got"], s["dec"]
    assert list(got) == ["emulator", "noise", "global", "local", "alpha"]
    assert got["local"].shape == (1, N) and all(got[k].shape == (N,) for k in got if k != "local")
    for k, key in enumerate(("emulator", "noise", "global")):
        np.testing.assert_array_equal(got[key], dec["comp"][0, k, 0])
    np.testing.assert_array_equal(got["local"][0], dec["comp"][0, 3, 0])
    np.testing.assert_array_equal(got["alpha"], dec["alpha"][0, 0])
    np.testing.assert_array_equal(got["alpha"], s["model"].cho_solve())


def test_components_add_up_to_the_residual():
    """r = flux - data.flux as the transform chain rounds it.  |sum - r| <= |C alpha - r| + |sum - C alpha|: the solve's
    bound of tests/test_gpu_apply_factor.py and the products' of tests/test_gpu_decompose.py, with the device's own
    matrix (SpectrumModel.__call__) for C."""
    s = shared()
    model, got = s["model"], s["got"]
    u = 2.0 ** -53
    gamma = lambda k: k * u / (1 - k * u)  # noqa: E731
    flux, cov = model()
    np.testing.assert_array_equal(flux, s["dec"]["flux"][0])
    r = flux - model.data.flux
    total = sum(got[k].astype(np.longdouble) for k in ("emulator", "noise", "global")) + got["local"][0]
    err = float(np.abs(total - r).max())
    a = np.abs(got["alpha"])
    bound = ((1e-13 + N * gamma(3 * N + 1)) * (np.abs(cov).sum(axis=1).max() * a.max() + np.abs(r).max())
             + (1e-13 + gamma(N + 4 + 4)) * (np.abs(cov) @ a).max())
    print(f"|sum of the components - r|_inf = {err:.3g}, bound {bound:.3g}")
    assert err <= bound


def test_right_hand_sides_of_both_ranks():
    s = shared()
    model = s["model"]
    rhs = np.random.default_rng(6).standard_normal((2, N))
    two = model.residual_components(rhs)
    assert two["local"].shape == (1, 2, N) and all(two[k].shape == (2, N) for k in two if k != "local")
    one = model.residual_components(rhs[1])
    np.testing.assert_array_equal(one["alpha"], model.cho_solve(rhs[1]))
    np.testing.assert_array_equal(two["alpha"], model.cho_solve(rhs))
    dev, md, rows = model._pack(update_caches=False)
    dec = dev.decompose(md, rows, rhs=rhs)
    for k, key in enumerate(("emulator", "noise", "global")):
        np.testing.assert_array_equal(two[key], dec["comp"][0, k])
    np.testing.assert_array_equal(two["local"], dec["comp"][0, 3:])


def test_the_models_state_is_left_alone():
    s = shared()
    model = synth.build_model(s["o"])
    l0 = model.log_likelihood()
    before = (len(model.residuals), model._lnprob, model._log_scale, model._glob_snapshot, model._loc_snapshot)
    model.residual_components()
    model.residual_components_batch(synth.walker_ball(s["o"], B=2, seed=3))
    assert (len(model.residuals), model._lnprob, model._log_scale, model._glob_snapshot, model._loc_snapshot) == before
    assert model.log_likelihood() == l0


def test_batch_rows_are_the_scalar_calls():
    s = shared()
    model = synth.build_model(s["o"])
    P = synth.walker_ball(s["o"], B=3, seed=3)
    P[1, synth.LABELS.index("T")] = 1e5  # outside the emulator grid
    got, info = model.residual_components_batch(P, return_info=True)
    assert list(got) == ["emulator", "noise", "global", "local", "alpha"] and list(info) == [0, -1, 0]
    assert got["local"].shape == (3, 1, N) and got["alpha"].shape == (3, N)
    assert all(np.isnan(got[k][1]).all() for k in got)
    for b in (0, 2):
        model.set_param_vector(P[b])
        one = model.residual_components()
        for key in got:
            np.testing.assert_array_equal(got[key][b], one[key])
    model.set_param_vector(P[1])
    with pytest.raises(ValueError):
        model.residual_components()
