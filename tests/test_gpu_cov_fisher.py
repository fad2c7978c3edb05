"""sf_fisher_cov_batch through DeviceOrder.fisher_cov and the SpectrumModel methods: the Fisher information of the covariance
hyper-parameters, F_ij = 1/2 tr(W D_i W D_j) with W = C^-1 and D_i = dC / d theta_i.

Cases: those of tests/test_gpu_gradient.py, parameter construction restated.  N180 (npad 192: the factorisation's shifted frame,
a partial last block, the local patch straddles the block boundary at 64), N256, N330, N180-two-local (no global kernel, the
second patch clipped by the order's end), N180-global; m = 4, the three walkers of walker_ball(seed=3).

The entry bound.  The device forms What = W + dW, T_j = fl(What Dhat_j), S_j = fl(T_j What) and F_ij = 1/2 fl(sum Dhat_i o S_j),
where Dhat is the derivative entry as the device evaluates it, |Dhat - D| <= 1e-13 Dbar (the fill's entry contract applied to
the derivative formulas; Dbar: the absolute value taken term by term).  With u = 2^-53 and gamma_k = k u / (1 - k u), to first
order in dW and u, against the longdouble reference of the oracle's matrix plus jitter:
  (1) 1/2 sum (|dW| Dbar_i |W| + |W| Dbar_i |dW|) o Dbar_j, the perturbation of the two factors W (by the cyclic trace this is
      the same number with i and j exchanged), with |dW| the |dG| of tests/test_gpu_gradient.py from the device's own factor L,
      X = L^-1: |dW| = |W| dC |W| + gamma_2n (E + E^T) + gamma_{n+1} |X|^T |X|, dC = 1e-13 |C| + gamma_{n+1} |L||L|^T,
      E = |X|^T |X||L||X|, n = npad (fill, factorisation, tile);
  (2) three roundings for each of the three products (W D_j, T_j W, D_i o S_j): 9 u size_ij;
  (3) the entry contract once per derivative factor: 2e-13 size_ij;
  (4) gamma_k size_ij with k the longest chain of sums: a tile of T_j sums at most npad products, a tile of S_j at most npad,
      and the contraction 16 per thread, 6 shuffle steps, 3 adds over the waves, at most nbr pairs of a block row (each times
      its weight: one rounding more) and nbr block rows: k = 2 npad + 3 nbr + 25, nbr = npad / 64;
with size_ij = 1/2 sum (|W| Dbar_i |W|) o Dbar_j.  The matrix products of the bound itself are evaluated in float64.  A
wrong-weight guard on top: every entry agrees with the float64 numpy reference to 1e-6 size_ij (a doubled diagonal pair or a
dropped symmetric half is off by order 1e-1 on the diagonal entries)."""
import numpy as np
import pytest

from oracle import sf_oracle as O
from starfish_amd import synth

import cov_derivatives as CD
import cov_fisher_reference as CF
from gpu_helpers import device_order, oracle_order, pack_rows

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
CASES = ["N180", "N256", "N330", "N180-two-local", "N180-global"]


def gamma(k):
    return k * U / (1 - k * U)


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
        c["out"] = do.fisher_cov(md, rows)
        _CASES[name] = c
    return _CASES[name]


@pytest.mark.parametrize("name", CASES)
def test_lnl_and_info_have_the_bits_of_loglike_and_the_matrix_is_finite_and_symmetric(name):
    c = case(name)
    do, md, rows, out = c["do"], c["md"], c["rows"], c["out"]
    s = (2 if md.has_global else 0) + 3 * md.n_local
    assert out["fisher"].shape == (3, s, s) and out["lnl"].shape == (3,)
    ll = do.loglike(md, rows)
    assert (ll["info"] == 0).all()
    np.testing.assert_array_equal(out["lnl"], ll["lnl"])
    np.testing.assert_array_equal(out["info"], ll["info"])
    assert np.isfinite(out["fisher"]).all()
    np.testing.assert_array_equal(out["fisher"], np.transpose(out["fisher"], (0, 2, 1)))
    assert (np.diagonal(out["fisher"], axis1=1, axis2=2) > 0).all()


@pytest.mark.parametrize("name", CASES)
def test_every_entry_within_its_bound_of_the_longdouble_reference(name):
    c = case(name)
    do, md, rows, oo, N = c["do"], c["md"], c["rows"], c["oo"], c["N"]
    npad = do.npad
    nbr = npad // 64
    k = 2 * npad + 3 * nbr + 25
    fac = do.apply(md, rows, "L", rhs=np.eye(N))  # L e_j sums one product by 1 and zeros: the factor, exactly
    assert (fac["info"] == 0).all()
    Ldev = np.transpose(fac["out"], (0, 2, 1))
    wave = c["o"]["wave"]
    worst = 0.0
    for b, p in enumerate(c["plist"]):
        C64 = O.forward_model(oo, p)[1] + 1e-10 * np.eye(N)
        W = CF.cinv(C64)
        named = CD.slot_derivatives(wave, p, dtype=LD)
        Dbar = [d for _, d in CD.slot_derivatives(wave, p, absolute=True)]
        D64 = [d for _, d in CD.slot_derivatives(wave, p)]
        ref = CF.contract(W, [d for _, d in named])
        ref64 = CF.fisher_cov(C64, D64, np.float64)
        # the pieces of the bound
        aL, aW = np.abs(Ldev[b]), np.abs(W).astype(np.float64)
        dC = 1e-13 * np.abs(C64) + gamma(npad + 1) * (aL @ aL.T)
        aX = np.abs(CF.inverse_longdouble(Ldev[b].astype(LD))).astype(np.float64)
        E = aX.T @ (aX @ (aL @ aX))
        dW = aW @ dC @ aW + gamma(2 * npad) * (E + E.T) + gamma(npad + 1) * (aX.T @ aX)
        size = CF.size(W, Dbar)
        s = len(named)
        assert c["out"]["fisher"].shape[1] == s
        for i in range(s):
            first_i = dW @ Dbar[i] @ aW + aW @ Dbar[i] @ dW
            for j in range(s):
                got = c["out"]["fisher"][b, i, j]
                bound = 0.5 * np.sum(first_i * Dbar[j]) + (9 * U + 2e-13 + gamma(k)) * size[i, j]
                err = abs(float(got - ref[i, j]))
                worst = max(worst, err / bound)
                if j <= i:
                    print(f"{name} walker {b} ({named[i][0]}, {named[j][0]}): {got!r}, err / bound = {err / bound:.3g} (bound {bound:.3g}), "
                          f"|got - float64 reference| / size = {abs(got - ref64[i, j]) / size[i, j]:.3g}")
                assert err <= bound, (name, b, i, j, got, float(ref[i, j]), err, bound)
                assert abs(got - ref64[i, j]) <= 1e-6 * size[i, j], (name, b, i, j, got, ref64[i, j], size[i, j])
    print(f"{name}: largest err / bound {worst:.3g}")


def test_chunked_and_repeated_calls_give_the_same_bits_and_the_workspace_has_the_documented_layout():
    c = case("N180")
    do, md, rows = c["do"], c["md"], c["rows"]
    for other in (do.fisher_cov(md, rows), do.fisher_cov(md, rows, max_chunk=1)):
        for key in ("lnl", "fisher", "info"):
            np.testing.assert_array_equal(other[key], c["out"][key], err_msg=key)
    sub = do.fisher_cov(md, rows[1:])
    np.testing.assert_array_equal(sub["fisher"], c["out"]["fisher"][1:])
    assert do.npad == 192 and -(-do.n // 64) == 3
    assert do.fisher_cov_workspace_bytes(md, 0) == 0
    sizes = np.array([do.fisher_cov_workspace_bytes(md, B) for B in (1, 2, 3, 64)])
    assert (np.diff(sizes) > 0).all()
    ld = 64 * -(-do.n // 64)
    for B in (1, 3, 64):
        # behind the gradient's layout: all of W and one T_j, ld x ld doubles per walker each (multiples of 256 bytes)
        assert do.fisher_cov_workspace_bytes(md, B) - do.loglike_grad_workspace_bytes(md, B) == 2 * 8 * B * ld * ld, B
    # the part quadratic in npad does not grow with the slots: s = 2 against s = 6 at the same npad
    extra = []
    for name, s in (("N180-global", 2), ("N180-two-local", 6)):
        q = case(name)
        assert (2 if q["md"].has_global else 0) + 3 * q["md"].n_local == s and q["do"].npad == 192
        extra.append(q["do"].fisher_cov_workspace_bytes(q["md"], 3) - q["do"].loglike_grad_workspace_bytes(q["md"], 3))
    assert extra[0] == extra[1] == 2 * 8 * 3 * 192 * 192


def test_failed_walkers_get_nan_matrices_and_leave_the_others_alone():
    """The mixed batch of tests/test_gpu_gradient.py: data without pixel noise and log_scale 18 (not positive definite),
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
    good, info0 = model.covariance_fisher_information_batch(P, return_info=True)
    assert (info0 == 0).all() and np.isfinite(good).all()
    got, info = model.covariance_fisher_information_batch(mixed, return_info=True)
    _, info_ll = model.log_likelihood_batch(mixed, return_info=True)
    np.testing.assert_array_equal(info, info_ll)
    assert info[1] > 0 and info[3] == -1 and (info[[0, 2, 4]] == 0).all(), info
    assert np.isnan(got[[1, 3]]).all()
    np.testing.assert_array_equal(got[[0, 2, 4]], good)
    model.set_param_vector(not_pd)
    with pytest.raises(np.linalg.LinAlgError, match="leading minor"):
        model.covariance_fisher_information()
    model.set_param_vector(off_grid)
    with pytest.raises(ValueError):
        model.covariance_fisher_information()


def test_model_methods_select_the_thawed_labels_and_parameter_covariance_inverts_the_matrix():
    c = case("N180")
    model = synth.build_model(c["o"])
    l0 = model.log_likelihood()
    before = (len(model.residuals), model._lnprob, model._log_scale, model._glob_snapshot, model._loc_snapshot)
    every = ("global_cov:log_amp", "global_cov:log_ls", "local_cov:0:mu", "local_cov:0:log_amp", "local_cov:0:log_sigma")
    assert model.gradient_labels == every
    dev, md, rows = model._pack(c["P"], update_caches=False)
    raw = dev.fisher_cov(md, rows)
    np.testing.assert_array_equal(model.covariance_fisher_information_batch(c["P"]), raw["fisher"])
    np.testing.assert_array_equal(raw["lnl"], model.log_likelihood_batch(c["P"]))
    dev, md, rows = model._pack(update_caches=False)
    F = model.covariance_fisher_information()
    np.testing.assert_array_equal(F, dev.fisher_cov(md, rows)["fisher"][0])
    # the Laplace covariance of every thawed label
    labels = model.fisher_labels
    assert labels == synth.LABELS
    cov = model.parameter_covariance(include_covariance=True)
    assert cov.shape == (13, 13) and np.isfinite(cov).all() and np.array_equal(cov, cov.T)
    assert np.linalg.eigvalsh(cov / np.sqrt(np.outer(np.diag(cov), np.diag(cov)))).min() > 0
    idx = [labels.index(k) for k in every]
    d = np.sqrt(np.diag(F))
    block = cov[np.ix_(idx, idx)] * np.outer(d, d)  # normalised: (D^-1 F D^-1)^-1
    eig = np.linalg.eigvalsh(F / np.outer(d, d))
    print("normalised eigenvalues of the covariance Fisher matrix:", eig)
    assert np.abs(block @ (F / np.outer(d, d)) - np.eye(5)).max() <= 1e-10
    mean_idx = [labels.index(k) for k in model.mean_gradient_labels]
    assert (cov[np.ix_(mean_idx, idx)] == 0).all()
    # frozen labels drop their rows and columns
    model.freeze(["local_cov:0:mu", "global_cov:log_ls"])
    assert model.gradient_labels == (every[0], every[3], every[4])
    keep = [i for i, k in enumerate(synth.LABELS) if k not in ("local_cov:0:mu", "global_cov:log_ls")]
    dev, md, rows = model._pack(c["P"][:, keep], update_caches=False)
    raw = dev.fisher_cov(md, rows)
    np.testing.assert_array_equal(model.covariance_fisher_information_batch(c["P"][:, keep]), raw["fisher"][:, [0, 3, 4]][:, :, [0, 3, 4]])
    model.thaw(["local_cov:0:mu", "global_cov:log_ls"])
    assert (len(model.residuals), model._lnprob, model._log_scale, model._glob_snapshot, model._loc_snapshot) == before
    assert model.log_likelihood() == l0
