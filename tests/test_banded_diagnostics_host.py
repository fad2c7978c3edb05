"""Host side of the residual diagnostics on the band solver: the identities the kernels evaluate (tests/
banded_diagnostics_reference.py, which tests/test_gpu_banded_diagnostics.py imports as its reference) against a dense inverse
on a random band + rank-m matrix; how DeviceOrder.diagnose_banded cuts right-hand sides into calls; what the Python layers refuse
and what they hand to the device, against tests/stand_in.py."""
import numpy as np
import pytest

from starfish_amd import _device as D

import banded_diagnostics_reference as BR
from stand_in import StandIn as HostStandIn, model_on_a_stand_in, state_of


def band_plus_rank_m(rng, n, w, m):
    """A strictly diagonally dominant band matrix of half-width w, and m rows Y."""
    A = np.zeros((n, n))
    for d in range(1, w + 1):
        v = rng.uniform(-1, 1, n - d)
        A += np.diag(v, d) + np.diag(v, -d)
    A += np.diag(np.abs(A).sum(axis=1) + rng.uniform(0.5, 1.5, n))
    return A, rng.standard_normal((m, n))


@pytest.mark.parametrize("n,w,m,k", [(40, 5, 3, 1), (57, 9, 4, 2), (64, 3, 17, 13), (33, 32, 2, 30)])
def test_identities_against_a_dense_inverse(n, w, m, k):
    rng = np.random.default_rng(1000 * n + k)
    Bd, Y = band_plus_rank_m(rng, n, w, m)
    R = rng.standard_normal((k, n))
    Cinv = np.linalg.inv(Bd + Y.T @ Y)
    q = BR.sweep(Bd, Y, R)
    assert q["T"].shape == (n, k + m) and q["G"].shape == (k + m, k + m)
    np.testing.assert_allclose(q["G"], q["G"].T, rtol=0, atol=1e-12 * np.abs(q["G"]).max())
    scale = np.abs(Cinv).max()
    Vs = BR.vs(q["T"], q["G"], k)
    np.testing.assert_allclose(q["Sigma"] - Vs @ Vs.T, Cinv, rtol=0, atol=1e-12 * scale)
    np.testing.assert_allclose(BR.cinv_diag(np.diag(q["Sigma"]), Vs), np.diag(Cinv), rtol=1e-11, atol=0)
    alpha = BR.mix(q["T"], q["G"], k)
    assert alpha.shape == (k, n)
    np.testing.assert_allclose(alpha, R @ Cinv, rtol=0, atol=1e-12 * np.abs(R @ Cinv).max())
    # the same in long double, as the GPU tests use it
    ql = BR.sweep(Bd.astype(np.longdouble), Y, R)
    assert ql["T"].dtype == np.longdouble
    np.testing.assert_allclose(BR.mix(ql["T"], ql["G"], k).astype(np.float64), alpha, rtol=0, atol=1e-12 * np.abs(alpha).max())
    assert BR.amplification(Bd, Y) > 0


def test_right_hand_sides_are_cut_into_groups_of_max_nrhs():
    assert D.rhs_groups(1, 28) == [(0, 1)]
    assert D.rhs_groups(28, 28) == [(0, 28)]
    assert D.rhs_groups(30, 28) == [(0, 28), (28, 30)]
    assert D.rhs_groups(30, 13) == [(0, 13), (13, 26), (26, 30)]
    for nrhs, cap in ((0, 5), (3, 0), (3, -1)):
        with pytest.raises(ValueError):
            D.rhs_groups(nrhs, cap)
    assert D.diagnose_wants("alpha") == ("alpha",) and D.diagnose_wants(()) == ("alpha",)
    assert D.diagnose_wants(("comp", "cov_diag")) == ("alpha", "cov_diag", "comp")
    with pytest.raises(ValueError, match="want"):
        D.diagnose_wants(("alpha", "L"))


class StandIn(HostStandIn):
    """The three dense calls as they were (no ``solver`` argument: a call that hands one over fails) and the same with one."""

    def _result(self, call, rows, rhs, want_flux, solver):
        B = rows.shape[0]
        k = 1 if rhs is None else np.asarray(rhs).shape[-2]
        self.calls.append((call, B, k, solver))
        out = dict(info=np.full(B, self.info, dtype=np.int32), alpha=np.ones((B, k, self.n)), out=np.ones((B, k, self.n)),
                   cinv_diag=np.ones((B, self.n)), cov_diag=np.ones((B, self.n)), comp=np.ones((B, 4, k, self.n)))
        if want_flux:
            out["flux"] = np.zeros((B, self.n))
        return out


class Dense(StandIn):
    def apply(self, md, rows, op, rhs=None, want_flux=False, max_chunk=None):
        return self._result("apply:" + op, rows, rhs, want_flux, None)

    def decompose(self, md, rows, rhs=None, want_flux=False, max_chunk=None):
        return self._result("decompose", rows, rhs, want_flux, None)

    def pointwise(self, md, rows, rhs=None, want_flux=False, max_chunk=None):
        return self._result("pointwise", rows, rhs, want_flux, None)


class WithSolver(StandIn):
    def apply(self, md, rows, op, rhs=None, want_flux=False, max_chunk=None, solver="dense"):
        return self._result("apply:" + op, rows, rhs, want_flux, solver)

    def decompose(self, md, rows, rhs=None, want_flux=False, max_chunk=None, solver="dense"):
        return self._result("decompose", rows, rhs, want_flux, solver)

    def pointwise(self, md, rows, rhs=None, want_flux=False, max_chunk=None, solver="dense"):
        return self._result("pointwise", rows, rhs, want_flux, solver)


def test_solver_none_is_the_call_as_it_always_was():
    """A device layer without the ``solver`` argument still serves every method: None and "dense" hand nothing over."""
    for built_with in ("dense", "auto"):
        model, dev = model_on_a_stand_in(Dense, solver=built_with)
        P = np.tile(model.get_param_vector(), (2, 1))
        state = state_of(model)
        for solver in (None, "dense"):
            model.cho_solve(solver=solver)
            model.residual_components(solver=solver)
            model.pointwise(solver=solver)
            model.apply_factor_batch(P, "Cinv", solver=solver)
            model.apply_factor_batch(P, "Linv", solver=solver)
            model.residual_components_batch(P, solver=solver)
            model.pointwise_batch(P, solver=solver)
        model.whiten()
        model.draw(rng=1)
        assert [c[0] for c in dev.calls[:7]] == ["apply:Cinv", "decompose", "pointwise", "apply:Cinv", "apply:Linv", "decompose",
                                                 "pointwise"]
        assert all(c[3] is None for c in dev.calls)
        assert state_of(model) == state


def test_the_band_solvers_are_handed_to_the_device_layer():
    model, dev = model_on_a_stand_in(WithSolver)
    n = dev.n
    P = np.tile(model.get_param_vector(), (3, 1))
    state = state_of(model)
    for solver in ("banded", "auto"):
        del dev.calls[:]
        assert model.cho_solve(solver=solver).shape == (n,)
        assert model.cho_solve(np.zeros((2, n)), solver=solver).shape == (2, n)
        assert set(model.residual_components(solver=solver)) == {"emulator", "noise", "global", "local", "alpha"}
        assert model.pointwise(solver=solver)["z"].shape == (n,)
        assert model.apply_factor_batch(P, "Cinv", np.zeros((3, 5, n)), solver=solver).shape == (3, 5, n)
        assert model.residual_components_batch(P, solver=solver)["local"].shape == (3, 1, n)
        got, info = model.pointwise_batch(P, np.zeros((2, n)), return_info=True, solver=solver)
        assert got["loo_mean"].shape == (3, 2, n) and got["loo_std"].shape == (3, n) and (info == 0).all()
        assert dev.calls == [("apply:Cinv", 1, 1, solver), ("apply:Cinv", 1, 2, solver), ("decompose", 1, 1, solver),
                             ("pointwise", 1, 1, solver), ("apply:Cinv", 3, 5, solver), ("decompose", 3, 1, solver),
                             ("pointwise", 3, 2, solver)]
    assert state_of(model) == state


def test_refusals_of_the_model_layer():
    model, dev = model_on_a_stand_in(WithSolver)
    P = np.tile(model.get_param_vector(), (2, 1))
    for bad in ("band", "Dense", 1):
        for call in (lambda: model.cho_solve(solver=bad), lambda: model.residual_components(solver=bad),
                     lambda: model.pointwise(solver=bad), lambda: model.apply_factor_batch(P, "Cinv", solver=bad),
                     lambda: model.residual_components_batch(P, solver=bad), lambda: model.pointwise_batch(P, solver=bad)):
            with pytest.raises(ValueError, match="solver must be"):
                call()
    for op in ("L", "Linv", "LinvT"):
        for solver in ("banded", "auto"):
            with pytest.raises(ValueError, match="Cinv"):
                model.apply_factor_batch(P, op, solver=solver)
    with pytest.raises(ValueError, match="op must be"):
        model.apply_factor_batch(P, "C", solver="auto")
    assert dev.calls == []
    # whiten and draw take no solver: they stay on the dense factor
    with pytest.raises(TypeError):
        model.whiten(solver="auto")
    with pytest.raises(TypeError):
        model.draw(solver="auto")
    # a failed walker raises as log_likelihood does, whatever the solver
    model, dev = model_on_a_stand_in(WithSolver)
    dev.info = -1
    for solver in (None, "banded", "auto"):
        for call in (model.cho_solve, model.residual_components, model.pointwise):
            with pytest.raises(ValueError, match="emulator"):
                call(solver=solver)
    dev.info = D.INFO_BANDWIDTH
    with pytest.raises(ValueError, match="band"):
        model.pointwise(solver="banded")


class FakeOrder:
    """DeviceOrder.apply's argument checks need no device: they run before anything is packed."""
    apply = D.DeviceOrder.apply

    def diagnose_banded(self, md, params, rhs, want, **kw):
        self.seen = (want, kw)
        return dict(alpha=np.zeros((1, 1, 4)), info=np.zeros(1, dtype=np.int32))


def test_refusals_of_the_device_layer():
    do = FakeOrder()
    for op in ("L", "Linv", "LinvT", 0, 1, 2):
        for solver in ("banded", "auto"):
            with pytest.raises(ValueError, match="triangular factor"):
                do.apply(None, None, op, solver=solver)
    with pytest.raises(ValueError, match="solver must be"):
        do.apply(None, None, "Cinv", solver="band")
    out = do.apply(None, None, "Cinv", solver="auto", max_chunk=2)
    assert set(out) == {"out", "info"} and do.seen == (("alpha",), dict(want_flux=False, max_chunk=2, solver="auto"))
    out = do.apply(None, None, 3, solver="banded")
    assert do.seen[1]["solver"] == "banded"
    for name in ("pointwise", "decompose", "diagnose_banded"):
        with pytest.raises(ValueError, match="solver must be"):
            getattr(D.DeviceOrder, name)(do, None, None, solver="wide")
    with pytest.raises(ValueError, match="solver must be"):
        D.DeviceOrder.diagnose_banded(do, None, None, solver="dense")  # (the dense calls are apply / pointwise / decompose)
