"""sf_apply_batch through DeviceOrder.apply and the SpectrumModel methods cho_solve / whiten / draw / apply_factor_batch.

Orders: N = 180 (npad 192 = 64 mod 128: the factorisation's shifted frame) and N = 256, three walkers with different
parameters, a global and one local kernel.  The bounds are Higham's (Accuracy and Stability of Numerical Algorithms,
Thms 8.5 and 10.4; u = 2^-53, gamma_k = k u / (1 - k u)) plus the project's 1e-13 for the covariance fill (SURVEY 8 d)."""
import numpy as np
import pytest

from oracle import sf_oracle as O
from starfish_amd import synth

from gpu_helpers import device_order, oracle_order, pack_rows

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SQMAH_RTOL = 1e-11  # the project's contract for sqmah


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
        c["tr"] = do.transform(md, rows)
        c["ll"] = do.loglike(md, rows)
        assert (c["ll"]["info"] == 0).all()
        c["cinv"] = do.apply(md, rows, "Cinv", want_flux=True)
        _CASES[N] = c
    return _CASES[N]


def device_factor(do, md, rows):
    """The L the device applies, exactly: L e_j sums one product by 1 and zeros.  (B, n, n)."""
    out = do.apply(md, rows, "L", rhs=np.eye(do.n))
    assert (out["info"] == 0).all()
    return np.transpose(out["out"], (0, 2, 1)).astype(np.longdouble)


@pytest.mark.parametrize("N", [180, 256])
def test_cinv_of_the_residual_solves_the_oracles_system(N):
    c = case(N)
    out = c["cinv"]
    assert (out["info"] == 0).all() and out["out"].shape == (3, 1, N)
    np.testing.assert_array_equal(out["flux"], c["tr"]["flux"])  # the transform chain's flux, bit for bit
    fac = 1e-13 + N * gamma(3 * N + 1)
    for b, p in enumerate(c["plist"]):
        C_ref = O.forward_model(c["oo"], p)[1] + 1e-10 * np.eye(N)
        x, R = out["out"][b, 0], c["tr"]["resid"][b]
        lhs = np.abs(C_ref @ x - R).max()
        rhs = fac * (np.abs(C_ref).sum(axis=1).max() * np.abs(x).max() + np.abs(R).max())
        print(f"N={N} walker {b}: |C x - R|_inf = {lhs:.3g}, bound {rhs:.3g}")
        assert lhs <= rhs


@pytest.mark.parametrize("N", [180, 256])
def test_quadratic_forms_agree_with_the_likelihoods_sqmah(N):
    c = case(N)
    white = c["do"].apply(c["md"], c["rows"], "Linv")
    assert (white["info"] == 0).all()
    for b in range(3):
        sq = c["ll"]["sqmah"][b]
        xr = float(c["cinv"]["out"][b, 0] @ c["tr"]["resid"][b])
        ww = float(white["out"][b, 0] @ white["out"][b, 0])
        print(f"N={N} walker {b}: sqmah {sq!r}, x.R rel {abs(xr - sq) / sq:.3g}, |whiten|^2 rel {abs(ww - sq) / sq:.3g}")
        assert abs(xr - sq) <= SQMAH_RTOL * abs(sq)
        assert abs(ww - sq) <= SQMAH_RTOL * abs(sq)


@pytest.mark.parametrize("N", [180, 256])
def test_draws_whiten_back_to_their_normal_vectors(N):
    """d = fl(flux + y_c) with y_c the computed L Z, y = fl(d - flux), x = whiten(y).  Thm 8.5 for the product and for the
    substitution, one rounding for each of the two additions:
    |L (x - Z)| <= |L x - y| + |y - y_c| + |y_c - L Z| <= gamma_n |L| |x| + 2 u (|d| + |flux|) + gamma_n |L| |Z|."""
    c = case(N)
    model = synth.build_model(c["o"])
    dev, md, rows = model._pack(update_caches=False)
    L = device_factor(dev, md, rows)[0]
    Z = np.random.default_rng(11).standard_normal((5, N))
    lz = dev.apply(md, rows, "L", rhs=Z, want_flux=True)
    flux = lz["flux"][0]
    np.testing.assert_array_equal(flux, dev.transform(md, rows)["flux"][0])
    d = model.draw(z=Z)
    assert d.shape == (5, N)
    np.testing.assert_array_equal(d, flux + lz["out"][0])
    y = d - flux
    x = model.whiten(y)
    assert x.shape == (5, N)
    g, aL = np.longdouble(gamma(N)), np.abs(L)
    Xl, Zl = x.astype(np.longdouble).T, Z.astype(np.longdouble).T
    # each step on its own: the product and the substitution within Thm 8.5 for the device's L
    assert (np.abs(lz["out"][0].astype(np.longdouble).T - L @ Zl) <= g * (aL @ np.abs(Zl))).all()
    assert (np.abs(L @ Xl - y.astype(np.longdouble).T) <= g * (aL @ np.abs(Xl))).all()
    err = np.abs(L @ (Xl - Zl))
    bound = g * (aL @ (np.abs(Xl) + np.abs(Zl))) + 2 * U * (np.abs(d) + np.abs(flux)[None, :]).astype(np.longdouble).T
    print(f"N={N}: max |L (x - Z)| / bound = {float((err / bound).max()):.3g}, max |x - Z| = {np.abs(x - Z).max():.3g}")
    assert (err <= bound).all()
    q = np.einsum("kn,kn->k", y, model.cho_solve(y))
    zz = np.einsum("kn,kn->k", Z, Z)
    print(f"N={N}: max rel |y C^-1 y - |z|^2| = {np.abs(q / zz - 1).max():.3g}")
    assert (np.abs(q - zz) <= SQMAH_RTOL * zz).all()
    # shapes: (n,) in, (n,) out; size / rng draws
    assert model.whiten(y[0]).shape == (N,) and np.array_equal(model.whiten(y[0]), x[0])
    assert model.cho_solve().shape == (N,) and model.draw(rng=1).shape == (N,) and model.draw(size=2, rng=1).shape == (2, N)
    np.testing.assert_array_equal(model.draw(size=2, rng=5), model.draw(size=2, rng=np.random.default_rng(5)))


def _zero_noise_model(N):
    """The rejected walker of tests/test_gpu_model.py: data without pixel noise and a calibration log_scale of 18 make the
    rank-m term swamp the rest; the matrix is numerically singular and LAPACK stops at a leading minor."""
    o = dict(synth.make_order(N=N, m=4, seed=5))
    o["sigma"] = np.zeros(N)
    return o, synth.build_model(o)


def test_failed_walkers_get_nan_rows_and_leave_the_others_alone():
    N = 256
    o, model = _zero_noise_model(N)
    P = synth.walker_ball(o, B=3, seed=21)
    not_pd, off_grid = P[1].copy(), P[2].copy()
    not_pd[2] = 18.0
    off_grid[synth.LABELS.index("T")] = 1e5
    with pytest.raises(np.linalg.LinAlgError):
        O.log_likelihood(oracle_order(o), synth.vector_to_oracle_params(not_pd))
    mixed = np.stack([P[0], not_pd, P[1], off_grid, P[2]])
    rhs = np.random.default_rng(2).standard_normal((2, N))
    for op, r in (("Cinv", None), ("Linv", rhs)):
        good, info0 = model.apply_factor_batch(P, op, rhs=r, return_info=True)
        assert (info0 == 0).all() and np.isfinite(good).all()
        got, info = model.apply_factor_batch(mixed, op, rhs=r, return_info=True)
        assert got.shape == ((5, N) if r is None else (5, 2, N))
        assert info[1] > 0 and info[3] == -1 and (info[[0, 2, 4]] == 0).all(), info
        assert np.isnan(got[1]).all() and np.isnan(got[3]).all()
        np.testing.assert_array_equal(got[[0, 2, 4]], good)
    model.set_param_vector(not_pd)
    with pytest.raises(np.linalg.LinAlgError, match="leading minor"):
        model.cho_solve()
    model.set_param_vector(off_grid)
    with pytest.raises(ValueError):
        model.whiten()
    with pytest.raises(ValueError):
        model.apply_factor_batch(P, "cinv")


def test_the_diagnostics_leave_the_models_state_alone():
    c = case(256)
    model = synth.build_model(c["o"])
    l0 = model.log_likelihood()
    before = (len(model.residuals), model._lnprob, model._log_scale, model._glob_snapshot, model._loc_snapshot)
    x = model.cho_solve()
    model.whiten()
    model.draw(rng=0)
    assert np.isfinite(x).all()
    assert (len(model.residuals), model._lnprob, model._log_scale, model._glob_snapshot, model._loc_snapshot) == before
    assert model.log_likelihood() == l0


def test_chunked_calls_give_the_same_bits():
    c = case(180)
    rhs = np.random.default_rng(4).standard_normal((3, 2, 180))
    whole = c["do"].apply(c["md"], c["rows"], "Cinv", rhs=rhs, want_flux=True)
    parts = c["do"].apply(c["md"], c["rows"], "Cinv", rhs=rhs, want_flux=True, max_chunk=2)
    for key in ("out", "info", "flux"):
        np.testing.assert_array_equal(whole[key], parts[key])
    np.testing.assert_array_equal(c["do"].apply(c["md"], c["rows"], "Cinv", max_chunk=2)["out"], c["cinv"]["out"])


def test_workspace_is_the_likelihoods_plus_the_staging_area():
    c = case(180)
    do, md = c["do"], c["md"]
    assert do.npad == 192
    sizes = np.array([[do.apply_workspace_bytes(md, B, k) for k in (1, 2, 16, 17)] for B in (1, 2, 3, 64)])
    assert (np.diff(sizes, axis=0) > 0).all() and (np.diff(sizes, axis=1) > 0).all()
    a256 = lambda x: -(-x // 256) * 256  # noqa: E731
    for B, k in ((1, 1), (3, 17), (64, 2)):
        # behind the likelihood's layout: the staging area, lnl and info, each on a 256-byte boundary
        extra = do.apply_workspace_bytes(md, B, k) - do.workspace_bytes(md, B)
        assert extra == a256(8 * B * k * do.npad) + a256(8 * B) + a256(4 * B), (B, k, extra)
    assert do.apply_workspace_bytes(md, 0, 1) == 0 and do.apply_workspace_bytes(md, 1, 0) == 0
