"""sf_pointwise_batch through DeviceOrder.pointwise and SpectrumModel.pointwise / pointwise_batch: alpha = C^-1 rhs,
diag(C^-1) and diag(C) of the matrix that is factorised, and the leave-one-out quantities derived from them.

Orders: N = 180 (npad 192 = 64 mod 128: the factorisation's shifted frame, a partial last block), 256 (exact blocks) and 330
(npad 384: six column blocks), three walkers with different parameters, a global and one local kernel.  u = 2^-53,
gamma_k = k u / (1 - k u).  diag(C^-1) is held to
  (1) |d^ - d| <= 2 gamma_2n diag(|X|^T |X||L||X|) + gamma_{n+1} d, n = npad, against the longdouble inverse X of the device's
      own L (the bound of tests/test_gpu_potri_diag.py), and
  (2) that plus diag(|C^-1| (1e-13 |C| + gamma_{n+1} |L||L|^T) |C^-1|) against the oracle's matrix: L L^T = C + dC with
      |dC| <= 1e-13 |C| (the fill's contract) + gamma_{n+1} |L||L|^T (Higham, Accuracy and Stability of Numerical
      Algorithms, Thm 10.3), and (C + dC)^-1 - C^-1 = -C^-1 dC C^-1 to first order."""
import numpy as np
import pytest

from oracle import sf_oracle as O
from starfish_amd import synth

from gpu_helpers import device_order, oracle_order, pack_rows

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SIZES = [180, 256, 330]
DERIVED = ("alpha", "marginal_std", "loo_mean", "loo_std", "z", "log_density")


def gamma(k):
    return k * U / (1 - k * U)


_CASES = {}


def case(N):
    """Order, oracle order, DeviceOrder, walkers, rows and the device results every test of that size shares (made once,
    never written)."""
    if N not in _CASES:
        o = synth.make_order(N=N, m=4, seed=5)
        oo = oracle_order(o)
        do = device_order(oo)
        P = synth.walker_ball(o, B=3, seed=3)
        plist = [synth.vector_to_oracle_params(p) for p in P]
        md, rows = pack_rows(do, plist)
        c = dict(o=o, oo=oo, do=do, P=P, plist=plist, md=md, rows=rows)
        c["rhs"] = np.random.default_rng(N).standard_normal((3, 2, N))
        c["own"] = do.pointwise(md, rows, want_flux=True)
        c["given"] = do.pointwise(md, rows, rhs=c["rhs"])
        _CASES[N] = c
    return _CASES[N]


def device_factor(do, md, rows):
    """The L the device applies, exactly: L e_j sums one product by 1 and zeros.  (B, n, n)."""
    out = do.apply(md, rows, "L", rhs=np.eye(do.n))
    assert (out["info"] == 0).all()
    return np.transpose(out["out"], (0, 2, 1)).astype(np.longdouble)


def inverse_longdouble(L):
    """X = L^-1 by forward substitution, row by row, in the precision of L."""
    X = np.zeros_like(L)
    for i in range(L.shape[0]):
        row = -(L[i, :i] @ X[:i])
        row[i] += 1
        X[i] = row / L[i, i]
    return X


def cholesky_longdouble(A):
    L = np.zeros_like(A)
    for j in range(A.shape[0]):
        L[j, j] = np.sqrt(A[j, j] - L[j, :j] @ L[j, :j])
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def first_bound(L, X, npad):
    aX = np.abs(X)
    return (np.longdouble(2 * gamma(2 * npad)) * np.sum(aX * (aX @ np.abs(L) @ aX), axis=0)
            + np.longdouble(gamma(npad + 1)) * np.sum(X * X, axis=0))


@pytest.mark.parametrize("N", SIZES)
def test_alpha_is_apply_cinv_bit_for_bit(N):
    c = case(N)
    do, md, rows = c["do"], c["md"], c["rows"]
    for out, rhs, k in ((c["own"], None, 1), (c["given"], c["rhs"], 2)):
        assert (out["info"] == 0).all()
        assert out["alpha"].shape == (3, k, N) and out["cinv_diag"].shape == (3, N) and out["cov_diag"].shape == (3, N)
        ref = do.apply(md, rows, "Cinv", rhs=rhs, want_flux=True)
        np.testing.assert_array_equal(out["alpha"], ref["out"])
        np.testing.assert_array_equal(out["info"], ref["info"])
    np.testing.assert_array_equal(c["own"]["flux"], ref["flux"])
    # the two diagonals do not depend on the right-hand sides
    np.testing.assert_array_equal(c["own"]["cinv_diag"], c["given"]["cinv_diag"])
    np.testing.assert_array_equal(c["own"]["cov_diag"], c["given"]["cov_diag"])


@pytest.mark.parametrize("N", SIZES)
def test_cov_diag_is_the_diagonal_that_is_factorised(N):
    c = case(N)
    for b, p in enumerate(c["plist"]):
        ref = np.diag(O.forward_model(c["oo"], p)[1]) + 1e-10
        rel = np.abs(c["own"]["cov_diag"][b] / ref - 1).max()
        print(f"N={N} walker {b}: max rel |cov_diag - oracle| = {rel:.3g}")
        np.testing.assert_allclose(c["own"]["cov_diag"][b], ref, rtol=1e-13, atol=0)


@pytest.mark.parametrize("N", SIZES)
def test_cinv_diag_against_the_devices_own_factor_and_against_the_oracle(N):
    c = case(N)
    do = c["do"]
    npad = do.npad
    L = device_factor(do, c["md"], c["rows"])
    for b, p in enumerate(c["plist"]):
        got = c["own"]["cinv_diag"][b].astype(np.longdouble)
        X = inverse_longdouble(L[b])
        d = np.sum(X * X, axis=0)
        b1 = first_bound(L[b], X, npad)
        e1 = np.abs(got - d)
        print(f"N={N} walker {b}: own factor: max err / bound = {float((e1 / b1).max()):.3g}, "
              f"max rel err = {float((e1 / d).max()):.3g}")
        assert (e1 <= b1).all()
        C_ref = (O.forward_model(c["oo"], p)[1] + 1e-10 * np.eye(N)).astype(np.longdouble)
        Xr = inverse_longdouble(cholesky_longdouble(C_ref))
        Cinv = Xr.T @ Xr
        aL, aCi = np.abs(L[b]), np.abs(Cinv)
        dC = np.longdouble(1e-13) * np.abs(C_ref) + np.longdouble(gamma(npad + 1)) * (aL @ aL.T)
        b2 = np.sum((aCi @ dC) * aCi, axis=1) + b1
        e2 = np.abs(got - np.diag(Cinv))
        ratio = c["own"]["cov_diag"][b] * c["own"]["cinv_diag"][b]
        print(f"N={N} walker {b}: oracle: max err / bound = {float((e2 / b2).max()):.3g}, "
              f"max rel err = {float((e2 / np.diag(Cinv)).max()):.3g}; diag(C) diag(C^-1) in [{ratio.min():.3g}, {ratio.max():.3g}]")
        assert (e2 <= b2).all()
        assert (ratio >= 1 - 1e-12).all()  # (C)_ii (C^-1)_ii >= 1 for a positive definite matrix


def formulas(rhs, alpha, cinv_diag, cov_diag):
    d = cinv_diag[..., None, :]
    z = alpha / np.sqrt(d)
    return dict(alpha=alpha, marginal_std=np.sqrt(cov_diag), loo_mean=rhs - alpha / d, loo_std=1.0 / np.sqrt(cinv_diag), z=z,
                log_density=-0.5 * np.log(2.0 * np.pi / d) - 0.5 * z * z)


@pytest.mark.parametrize("N", SIZES)
def test_model_methods_apply_the_formulas_and_leave_the_state_alone(N):
    c = case(N)
    model = synth.build_model(c["o"])
    l0 = model.log_likelihood()
    before = (len(model.residuals), model._lnprob, model._log_scale, model._glob_snapshot, model._loc_snapshot)
    dev, md, rows = model._pack(update_caches=False)
    R = c["rhs"]
    for rhs, lead in ((None, ()), (R[0, 0], ()), (R[0], (2,))):
        raw = dev.pointwise(md, rows, rhs=None if rhs is None else np.atleast_2d(rhs), want_flux=True)
        r = (raw["flux"][0] - model.data.flux)[None, :] if rhs is None else np.atleast_2d(rhs)
        want = formulas(r, raw["alpha"][0], raw["cinv_diag"][0], raw["cov_diag"][0])
        got = model.pointwise(rhs)
        assert tuple(got) == DERIVED
        for key in DERIVED:
            per_matrix = key in ("marginal_std", "loo_std")
            assert got[key].shape == (() if per_matrix else lead) + (N,), key
            np.testing.assert_array_equal(got[key], want[key] if per_matrix or lead else want[key][0], err_msg=key)
        assert np.isfinite(got["log_density"]).all() and (got["loo_std"] <= got["marginal_std"] * (1 + 1e-12)).all()
    np.testing.assert_array_equal(model.pointwise()["alpha"], model.cho_solve())
    P = c["P"]
    dev, md, rows = model._pack(P, update_caches=False)
    for rhs, lead in ((None, ()), (R[0, 0], ()), (R[0], (2,)), (R, (2,))):
        shaped = None if rhs is None else (rhs if rhs.ndim == 3 else np.atleast_2d(rhs))
        raw = dev.pointwise(md, rows, rhs=shaped, want_flux=True)
        r = (raw["flux"] - model.data.flux)[:, None, :] if rhs is None else shaped
        want = formulas(r, raw["alpha"], raw["cinv_diag"], raw["cov_diag"])
        got, info = model.pointwise_batch(P, rhs, return_info=True)
        assert tuple(got) == DERIVED and (info == 0).all()
        for key in DERIVED:
            per_matrix = key in ("marginal_std", "loo_std")
            assert got[key].shape == (3,) + (() if per_matrix else lead) + (N,), key
            np.testing.assert_array_equal(got[key], want[key] if per_matrix or lead else want[key][:, 0], err_msg=key)
    for bad in (np.zeros(N - 1), np.zeros((2, N + 1)), np.zeros((1, 2, N))):
        with pytest.raises(ValueError):
            model.pointwise(bad)
    with pytest.raises(ValueError):
        model.pointwise_batch(P, np.zeros((2, 2, N)))
    assert (len(model.residuals), model._lnprob, model._log_scale, model._glob_snapshot, model._loc_snapshot) == before
    assert model.log_likelihood() == l0


def test_failed_walkers_get_nan_rows_and_leave_the_others_alone():
    """The mixed batch of tests/test_gpu_apply_factor.py: data without pixel noise and log_scale 18 (not positive definite),
    T = 1e5 (outside the grid)."""
    N = 256
    o = dict(synth.make_order(N=N, m=4, seed=5))
    o["sigma"] = np.zeros(N)
    model = synth.build_model(o)
    P = synth.walker_ball(o, B=3, seed=21)
    not_pd, off_grid = P[1].copy(), P[2].copy()
    not_pd[2] = 18.0
    off_grid[synth.LABELS.index("T")] = 1e5
    mixed = np.stack([P[0], not_pd, P[1], off_grid, P[2]])
    rhs = np.random.default_rng(2).standard_normal((2, N))
    for r in (None, rhs):
        good, info0 = model.pointwise_batch(P, r, return_info=True)
        assert (info0 == 0).all() and all(np.isfinite(v).all() for v in good.values())
        got, info = model.pointwise_batch(mixed, r, return_info=True)
        _, info_apply = model.apply_factor_batch(mixed, "Cinv", rhs=r, return_info=True)
        np.testing.assert_array_equal(info, info_apply)
        assert info[1] > 0 and info[3] == -1 and (info[[0, 2, 4]] == 0).all(), info
        for key in DERIVED:
            assert np.isnan(got[key][1]).all() and np.isnan(got[key][3]).all(), key
            np.testing.assert_array_equal(got[key][[0, 2, 4]], good[key], err_msg=key)
    dev, md, rows = model._pack(mixed, update_caches=False)
    raw = dev.pointwise(md, rows)
    for key in ("alpha", "cinv_diag", "cov_diag"):
        assert np.isnan(raw[key][[1, 3]]).all() and np.isfinite(raw[key][[0, 2, 4]]).all(), key
    model.set_param_vector(not_pd)
    with pytest.raises(np.linalg.LinAlgError, match="leading minor"):
        model.pointwise()
    model.set_param_vector(off_grid)
    with pytest.raises(ValueError):
        model.pointwise()


def test_chunked_calls_give_the_same_bits():
    c = case(180)
    do, md, rows = c["do"], c["md"], c["rows"]
    parts = do.pointwise(md, rows, rhs=c["rhs"], want_flux=True, max_chunk=2)
    whole = do.pointwise(md, rows, rhs=c["rhs"], want_flux=True)
    for key in ("alpha", "cinv_diag", "cov_diag", "info", "flux"):
        np.testing.assert_array_equal(whole[key], parts[key], err_msg=key)
        if key != "flux":
            np.testing.assert_array_equal(whole[key], c["given"][key], err_msg=key)
    own = do.pointwise(md, rows, max_chunk=2)
    for key in ("alpha", "cinv_diag", "cov_diag"):
        np.testing.assert_array_equal(own[key], c["own"][key], err_msg=key)


def test_workspace_grows_with_walkers_and_right_hand_sides():
    c = case(180)
    do, md = c["do"], c["md"]
    assert do.npad == 192
    sizes = np.array([[do.pointwise_workspace_bytes(md, B, k) for k in (1, 2, 16, 17)] for B in (1, 2, 3, 64)])
    assert (np.diff(sizes, axis=0) > 0).all() and (np.diff(sizes, axis=1) > 0).all()
    a256 = lambda x: -(-x // 256) * 256  # noqa: E731
    for B, k in ((1, 1), (3, 17), (64, 2)):
        # behind sf_apply_batch's layout: two rows of npad per walker, then the workspace of the inverse's launch
        extra = do.pointwise_workspace_bytes(md, B, k) - do.apply_workspace_bytes(md, B, k)
        assert extra == 2 * a256(8 * B * do.npad) + do.lib.sf_potri_diag_workspace_bytes(do.npad, B), (B, k, extra)
    assert do.pointwise_workspace_bytes(md, 0, 1) == 0 and do.pointwise_workspace_bytes(md, 1, 0) == 0
