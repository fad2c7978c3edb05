"""sf_loglike_grad_batch through DeviceOrder.loglike_grad and the SpectrumModel methods: the gradient of the likelihood in
the covariance hyper-parameters, d lnL / d theta = 1/2 sum_ij A_ij D_ij with A = alpha alpha^T - C^-1, D = dC / d theta.

Orders: N = 180 (npad 192: the factorisation's shifted frame, a partial last block, the local patch at N / 3 straddles the
block boundary at 64), 256 and 330, m = 4, the three walkers of walker_ball(seed=3), a global and one local kernel; at
N = 180 also two local kernels without a global one, the second within 2 sigma of the order's last pixel (clipped support),
and a global kernel alone.

Every slot is held to a derived bound against a np.longdouble reference built from the oracle's matrix plus jitter and the
device's own residual flux - data, with D from tests/cov_derivatives.py in longdouble.  u = 2^-53, gamma_k = k u / (1 - k u),
n = npad, L the device's own factor, X = L^-1, Dbar the derivative with the absolute value taken term by term:
  (1) 1/2 sum_ij (|dalpha|_i |alpha|_j + |alpha|_i |dalpha|_j + |dG|_ij) Dbar_ij with
      |dalpha| = |C^-1| dC |alpha| + |C^-1| e (1e-13 + N gamma_{3N+1}) (|C|_inf |alpha|_inf + |r|_inf)   (the solve's bound of
      tests/test_gpu_apply_factor.py), dC = 1e-13 |C| + gamma_{n+1} |L||L|^T (tests/test_gpu_pointwise.py), and
      |dG| = |C^-1| dC |C^-1| + gamma_2n (E + E^T) + gamma_{n+1} |X|^T |X|, E = |X|^T |X||L||X| (tests/test_gpu_potri_blocks.py);
  (2) 1/2 sum 3 u (|alpha_i alpha_j| + |G_ij|) Dbar_ij: the product, the difference and the product with D;
  (3) 1e-13 1/2 sum |A_ij| Dbar_ij: the fill's entry contract applied to the derivative formulas;
  (4) gamma_k 1/2 sum |A_ij| Dbar_ij with k the number of non-zero entries of D: any order of summation.
The matrix products of the bound itself are evaluated in float64.  A wrong-weight guard on top: the slots agree with the
float64 reference to 1e-6 relative to 1/2 sum |A| Dbar (a doubled diagonal block or a dropped symmetric half is off by order
1e-1)."""
import numpy as np
import pytest

from oracle import sf_oracle as O
from starfish_amd import synth

import cov_derivatives as CD
from gpu_helpers import device_order, oracle_order, pack_rows

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
CASES = ["N180", "N256", "N330", "N180-two-local", "N180-global"]


def gamma(k):
    return k * U / (1 - k * U)


def inverse_longdouble(L):
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


def oracle_params(o, name, vec):
    p = synth.vector_to_oracle_params(vec)
    if name.endswith("two-local"):
        w = o["wave"]
        n = len(w)
        del p["global_cov"]
        (mu, la, ls), = p["local_cov"]
        # 9.37 pixels (about 1.25 sigma at 15 km/s and 2 km/s pixels) inside the last pixel: the patch is clipped by the order's end
        p["local_cov"] = [(mu, la, ls), (float(w[n - 10] + 0.37 * (w[n - 9] - w[n - 10])), la - 0.3, ls + 0.02)]
    if name.endswith("global"):
        del p["local_cov"]
    return p


_CASES = {}


def case(name):
    """Order, DeviceOrder, rows and the device results every test of that case shares (made once, never written)."""
    if name not in _CASES:
        N = int(name[1:4])
        o = synth.make_order(N=N, m=4, seed=5)
        oo = oracle_order(o)
        do = device_order(oo)
        P = synth.walker_ball(o, B=3, seed=3)
        plist = [oracle_params(o, name, p) for p in P]
        md, rows = pack_rows(do, plist)
        c = dict(N=N, o=o, oo=oo, do=do, P=P, plist=plist, md=md, rows=rows)
        c["out"] = do.loglike_grad(md, rows, want_flux=True)
        _CASES[name] = c
    return _CASES[name]


@pytest.mark.parametrize("name", CASES)
def test_no_mu_sits_on_a_kink(name):
    """In mu the likelihood has a kink wherever two pixels of the patch are equidistant from it: the reference's derivative
    is the almost-everywhere one, so every mu keeps 1e-3 pixel from every pixel and every midpoint of two pixels."""
    c = case(name)
    w = c["o"]["wave"]
    mids = 0.5 * (w[:, None] + w[None, :])  # (the diagonal: the pixels themselves)
    for p in c["plist"]:
        for mu, _, _ in p.get("local_cov", []):
            k = int(np.clip(np.searchsorted(w, mu), 1, len(w) - 1))
            off = np.abs(mids - mu).min() / (w[k] - w[k - 1])
            print(f"{name}: mu = {mu:.4f} is {off:.3f} pixel from the nearest kink")
            assert off >= 1e-3


@pytest.mark.parametrize("name", CASES)
def test_lnl_info_and_flux_have_the_bits_of_loglike_and_apply(name):
    c = case(name)
    do, md, rows, out = c["do"], c["md"], c["rows"], c["out"]
    slots = (2 if md.has_global else 0) + 3 * md.n_local
    assert out["grad"].shape == (3, slots) and out["lnl"].shape == (3,) and out["flux"].shape == (3, c["N"])
    ll = do.loglike(md, rows)
    assert (ll["info"] == 0).all()
    np.testing.assert_array_equal(out["lnl"], ll["lnl"])
    np.testing.assert_array_equal(out["info"], ll["info"])
    np.testing.assert_array_equal(out["flux"], do.apply(md, rows, "Cinv", want_flux=True)["flux"])
    assert np.isfinite(out["grad"]).all()


@pytest.mark.parametrize("name", CASES)
def test_every_slot_within_its_bound_of_the_longdouble_reference(name):
    c = case(name)
    do, md, rows, oo, N = c["do"], c["md"], c["rows"], c["oo"], c["N"]
    npad = do.npad
    fac = do.apply(md, rows, "L", rhs=np.eye(N))  # L e_j sums one product by 1 and zeros: the factor, exactly
    assert (fac["info"] == 0).all()
    Ldev = np.transpose(fac["out"], (0, 2, 1))
    wave = c["o"]["wave"]
    for b, p in enumerate(c["plist"]):
        C64 = O.forward_model(oo, p)[1] + 1e-10 * np.eye(N)
        Xr = inverse_longdouble(cholesky_longdouble(C64.astype(LD)))
        Cinv = Xr.T @ Xr
        r64 = c["out"]["flux"][b] - oo.flux
        alpha = Cinv @ r64.astype(LD)
        A = np.outer(alpha, alpha) - Cinv
        # the pieces of the bound
        aL, aCi, aal, aA = np.abs(Ldev[b]), np.abs(Cinv).astype(np.float64), np.abs(alpha).astype(np.float64), np.abs(A).astype(np.float64)
        dC = 1e-13 * np.abs(C64) + gamma(npad + 1) * (aL @ aL.T)
        solve = (1e-13 + N * gamma(3 * N + 1)) * (np.abs(C64).sum(axis=1).max() * aal.max() + np.abs(r64).max())
        d_alpha = aCi @ (dC @ aal) + aCi.sum(axis=1) * solve
        aX = np.abs(inverse_longdouble(Ldev[b].astype(LD))).astype(np.float64)
        E = aX.T @ (aX @ (aL @ aX))
        dG = aCi @ dC @ aCi + gamma(2 * npad) * (E + E.T) + gamma(npad + 1) * (aX.T @ aX)
        first = np.outer(d_alpha, aal) + np.outer(aal, d_alpha) + dG
        second = 3 * U * (np.outer(aal, aal) + aCi)
        # the float64 reference of the wrong-weight guard
        A64 = np.outer(*(np.linalg.solve(C64, r64),) * 2) - np.linalg.inv(C64)
        D = CD.slot_derivatives(wave, p, dtype=LD)
        Dbar = CD.slot_derivatives(wave, p, absolute=True)
        D64 = CD.slot_derivatives(wave, p)
        assert len(D) == c["out"]["grad"].shape[1]
        for s, ((label, d), (_, dbar), (_, d64)) in enumerate(zip(D, Dbar, D64)):
            got = c["out"]["grad"][b, s]
            ref = 0.5 * np.sum(A * d)
            size = 0.5 * np.sum(aA * dbar)
            k = int(np.count_nonzero(dbar))
            bound = 0.5 * np.sum(first * dbar) + 0.5 * np.sum(second * dbar) + 1e-13 * size + gamma(k) * size
            err = abs(float(got - ref))
            ref64 = 0.5 * np.sum(A64 * d64)
            print(f"{name} walker {b} {label}: {got!r}, err / bound = {err / bound:.3g} (bound {bound:.3g}, {k} entries), "
                  f"|got - float64 reference| / (1/2 sum |A| Dbar) = {abs(got - ref64) / size:.3g}")
            assert err <= bound, (name, b, label, got, float(ref), err, bound)
            assert abs(got - ref64) <= 1e-6 * size, (name, b, label, got, ref64, size)


def test_chunked_and_repeated_calls_give_the_same_bits_and_the_workspace_grows_with_walkers():
    c = case("N180")
    do, md, rows = c["do"], c["md"], c["rows"]
    for other in (do.loglike_grad(md, rows, want_flux=True), do.loglike_grad(md, rows, want_flux=True, max_chunk=1)):
        for key in ("lnl", "grad", "info", "flux"):
            np.testing.assert_array_equal(other[key], c["out"][key], err_msg=key)
    assert do.npad == 192
    sizes = np.array([do.loglike_grad_workspace_bytes(md, B) for B in (1, 2, 3, 64)])
    assert (np.diff(sizes) > 0).all()
    a256 = lambda x: -(-x // 256) * 256  # noqa: E731
    slots = (2 if md.has_global else 0) + 3 * int(md.n_local)
    assert (do.npad // 64, -(-do.n // 64), slots) == (3, 3, 5)
    for B in (1, 3, 64):
        # behind sf_apply_batch's layout with one right-hand side: a row of npad per walker, the workspace of the inverse's
        # launch (the three block inverses), then 3 block rows x 5 slots per walker
        extra = do.loglike_grad_workspace_bytes(md, B) - do.apply_workspace_bytes(md, B, 1)
        assert extra == (a256(8 * B * do.npad) + do.lib.sf_potri_diag_workspace_bytes(do.npad, B)
                         + a256(8 * B * -(-do.n // 64) * slots)), (B, extra)
        assert do.lib.sf_potri_diag_workspace_bytes(do.npad, B) >= 8 * B * 3 * 64 * 64
    assert do.loglike_grad_workspace_bytes(md, 0) == 0


def test_failed_walkers_get_nan_rows_and_leave_the_others_alone():
    """The mixed batch of tests/test_gpu_pointwise.py: data without pixel noise and log_scale 18 (not positive definite),
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
    lnl0, good, info0 = model.log_likelihood_gradient_batch(P, return_info=True)
    assert (info0 == 0).all() and np.isfinite(good).all() and np.isfinite(lnl0).all()
    lnl, got, info = model.log_likelihood_gradient_batch(mixed, return_info=True)
    _, info_ll = model.log_likelihood_batch(mixed, return_info=True)
    np.testing.assert_array_equal(info, info_ll)
    assert info[1] > 0 and info[3] == -1 and (info[[0, 2, 4]] == 0).all(), info
    assert np.isnan(got[[1, 3]]).all() and np.isneginf(lnl[[1, 3]]).all()
    np.testing.assert_array_equal(got[[0, 2, 4]], good)
    np.testing.assert_array_equal(lnl[[0, 2, 4]], lnl0)
    dev, md, rows = model._pack(mixed, update_caches=False)
    raw = dev.loglike_grad(md, rows)
    assert np.isnan(raw["grad"][[1, 3]]).all() and np.isfinite(raw["grad"][[0, 2, 4]]).all()
    model.set_param_vector(not_pd)
    with pytest.raises(np.linalg.LinAlgError, match="leading minor"):
        model.log_likelihood_gradient()
    model.set_param_vector(off_grid)
    with pytest.raises(ValueError):
        model.log_likelihood_gradient()


def test_model_methods_return_the_columns_of_the_thawed_labels():
    c = case("N180")
    model = synth.build_model(c["o"])
    l0 = model.log_likelihood()
    before = (len(model.residuals), model._lnprob, model._log_scale, model._glob_snapshot, model._loc_snapshot)
    every = ("global_cov:log_amp", "global_cov:log_ls", "local_cov:0:mu", "local_cov:0:log_amp", "local_cov:0:log_sigma")
    assert model.gradient_labels == every
    dev, md, rows = model._pack(c["P"], update_caches=False)
    raw = dev.loglike_grad(md, rows)
    lnl, g = model.log_likelihood_gradient_batch(c["P"])
    np.testing.assert_array_equal(lnl, raw["lnl"])
    np.testing.assert_array_equal(g, raw["grad"])
    np.testing.assert_array_equal(lnl, model.log_likelihood_batch(c["P"]))
    lnl1, g1 = model.log_likelihood_gradient()
    assert lnl1 == l0 and tuple(g1) == every
    dev, md, rows = model._pack(update_caches=False)
    np.testing.assert_array_equal(list(g1.values()), dev.loglike_grad(md, rows)["grad"][0])
    model.freeze(["local_cov:0:mu", "global_cov:log_ls"])
    assert model.gradient_labels == (every[0], every[3], every[4])
    keep = [i for i, k in enumerate(synth.LABELS) if k not in ("local_cov:0:mu", "global_cov:log_ls")]
    dev, md, rows = model._pack(c["P"][:, keep], update_caches=False)
    raw = dev.loglike_grad(md, rows)
    lnl, g = model.log_likelihood_gradient_batch(c["P"][:, keep])
    np.testing.assert_array_equal(g, raw["grad"][:, [0, 3, 4]])
    model.thaw(["local_cov:0:mu", "global_cov:log_ls"])
    assert (len(model.residuals), model._lnprob, model._log_scale, model._glob_snapshot, model._loc_snapshot) == before
    assert model.log_likelihood() == l0


def test_train_covariance_climbs_from_displaced_hyperparameters():
    c = case("N180")
    model = synth.build_model(c["o"])
    for key in ("global_cov:log_amp", "global_cov:log_ls", "local_cov:0:log_amp", "local_cov:0:log_sigma"):
        model[key] = model[key] + 0.5
    others = {k: model[k] for k in model.labels if k not in model.gradient_labels}
    start = model.log_likelihood()
    soln = model.train_covariance()
    print(f"train_covariance: {soln.message}; nit {soln.nit}, nfev {soln.nfev}; lnL {start!r} -> {-soln.fun!r}")
    assert soln.success, soln.message
    assert soln.x.shape == (len(model.gradient_labels),)
    np.testing.assert_array_equal([model[k] for k in model.gradient_labels], soln.x)
    assert {k: model[k] for k in others} == others
    assert model.log_likelihood() == -soln.fun
    assert -soln.fun > start
