"""The residual diagnostics on the band + Woodbury solver: sf_diagnose_banded_batch through DeviceOrder.diagnose_banded, the
``solver`` argument of DeviceOrder.apply / pointwise / decompose and of the SpectrumModel methods.

Cases: those of tests/test_gpu_banded_cov_gradient.py (N180: npad 192 and a partial last block; N256; N330; two local kernels;
global only; m = 17; a narrow global kernel, where the window slides), three walkers each, with k = the walker's own residual,
2 (per walker), 13 (shared; m + 13 rows are two blocks of right-hand sides) and 30 (per walker).  At the half-widths of the
wide cases (113 .. 128: two blocks, 32 rows) 30 right-hand sides go in two calls, which the test asserts; in N330-narrow they
are one call with three blocks.  Every walker's host bound fits the window and every walker comes back with info == 0, which
every test asserts: no case may pass by falling back.

u = 2^-53, gamma_k = k u / (1 - k u).  Every bound is evaluated from the oracle's matrices and their np.longdouble factors
alone (tests/banded_diagnostics_reference.py, tests/banded_derivatives.pieces: C = Bd + Y^T Y).

alpha      |C x - R|_inf <= fac (||C||_inf ||x||_inf + ||R||_inf), fac = 1e-13 + N gamma_{3N+1}: the check of
           tests/test_gpu_apply_factor.py::test_cinv_of_the_residual_solves_the_oracles_system, against the oracle's matrix.
           The dense call goes through the same check as the yardstick; both ratios are printed.  The Woodbury identity is
           not backward stable in general (the bound would then gain ||Bd^-1|| ||Y^T Y||, tests/banded_diagnostics_reference.
           amplification, printed beside the ratios: 0.36 .. 0.48 here); it is not needed: the largest ratio seen is 2.4e-4
           for the band call (N180-two-local) and 1.2e-2 for the dense one (N180-global), and the bound stands as it is.
cov_diag   rtol 1e-13 against the oracle's diagonal plus the jitter: the fill's contract.
cinv_diag  against the longdouble inverse of the oracle's matrix: bound (2) of tests/test_gpu_pointwise.py with L the
           longdouble factor of C (as tests/test_gpu_banded_cov_gradient.py takes it), plus selinv_bound's diagonal for
           Sigma_ii = (Bd^-1)_ii, plus the cancellation term gamma_c (Sigma_ii + sum_c Vs_ic^2) with c = m + 1: m products, m - 1
           additions and one subtraction, each rounded once (a fused multiply-add rounds less).  The dense call goes through
           the same check; both fractions are printed.  cov_diag * cinv_diag >= 1 - 1e-12.
           Seen: at most 2.1e-2 of the bound for the band call (N180-two-local; 2.5e-3 elsewhere), 0.27 .. 0.41 for the dense
           call in the cases with the wide global kernel and 2.4 in N330-narrow: bound (2) takes |dC| <= 1e-13 |C| for the fill,
           which the likelihood's table of the global kernel per diagonal (log-uniform grids; off by the rounding of the grid,
           ~3e-11 in r) does not keep for a narrow kernel.  sf_diagnose_banded_batch therefore fills its band entry by entry.
comp       ratio_to_bound of tests/test_gpu_decompose.py for the global and every local kernel, its noise row and its sum
           identity sum_k comp_k = (C + jitter) alpha, with that file's bounds."""
import numpy as np
import pytest

from oracle import sf_oracle as O
from starfish_amd import _device as D
from starfish_amd import _lib, synth

import banded_derivatives as BD
import banded_diagnostics_reference as BR
import band_selinv_reference as SR
from test_gpu_banded_cov_gradient import CASES, case as base_case
from test_gpu_decompose import structured_ratios, sum_ratio
from test_gpu_pointwise import first_bound

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
KS = ("own", 2, 13, 30)
ALL = ("alpha", "cinv_diag", "cov_diag", "comp")
SENTINEL = -7.0


def gamma(k):
    return k * U / (1 - k * U)


_CASES = {}


def rhs_of(name, k, N):
    """The right-hand sides of a case: None (own), (3, k, N) per walker for k = 2 and 30, (13, N) shared."""
    if k == "own":
        return None
    rng = np.random.default_rng(1000 * CASES.index(name) + k)
    return rng.standard_normal((13, N)) if k == 13 else rng.standard_normal((3, k, N))


def case(name):
    """The base case (order, DeviceOrder, rows) with the device results every test here shares (made once, never written)."""
    if name not in _CASES:
        b = base_case(name)
        do, md, rows = b["do"], b["md"], b["rows"]
        c = dict(b)
        c["W"] = int(b["hw"].max())
        c["kmax"] = do.diagnose_banded_max_nrhs(c["W"])
        c["rhs"] = {k: rhs_of(name, k, b["N"]) for k in KS}
        c["band"] = {k: do.diagnose_banded(md, rows, c["rhs"][k], want=ALL, want_flux=True) for k in KS}
        c["pointwise"] = {k: do.pointwise(md, rows, c["rhs"][k]) for k in ("own", 2)}
        c["decompose"] = {k: do.decompose(md, rows, c["rhs"][k]) for k in ("own", 2)}
        c["tr"] = do.transform(md, rows)
        c["cov"] = do.forward(md, rows)["cov"]
        _CASES[name] = c
    return _CASES[name]


def reference(c, b):
    """The oracle's matrices of walker b and what the bounds need of their longdouble factors (made once per walker)."""
    key = ("diag-ref", b)
    if key not in c:
        q = BD.pieces(c["oo"], c["plist"][b])
        C64, Bd64, Y64 = q["C"], q["Bd"], q["Y"]
        L = BR.cholesky(C64.astype(LD))
        X = BR.inverse_lower(L)
        LB = BR.cholesky(Bd64.astype(LD))
        XB = BR.inverse_lower(LB)
        TY = XB.T @ (XB @ Y64.T.astype(LD))             # Bd^-1 Y^T
        S = np.eye(Y64.shape[0], dtype=LD) + Y64.astype(LD) @ TY
        Vs = TY @ BR.inverse_lower(BR.cholesky(S)).T
        c[key] = dict(C=C64, Bd=Bd64, Y=Y64, L=L, X=X, LB=LB, sigma_diag=np.sum(XB * XB, axis=0), Vs=Vs,
                      cinv_diag=np.sum(X * X, axis=0))
    return c[key]


def rhs_rows(c, k, b):
    """The right-hand sides of walker b as (k, N): its own residual from the transform chain, or the given ones."""
    if k == "own":
        return c["tr"]["resid"][b][None, :]
    r = c["rhs"][k]
    return r[b] if r.ndim == 3 else r


@pytest.mark.parametrize("name", CASES)
def test_every_case_runs_on_the_band_solver(name):
    c = case(name)
    do, N, m = c["do"], c["N"], c["m"]
    print(name, "half-width bounds", c["hw"], "window", do.banded_window_halfwidth(), "max_nrhs", c["kmax"])
    assert c["hw"].max() <= do.banded_window_halfwidth() <= 144
    nl = int(c["md"].n_local)
    for k in KS:
        out, kk = c["band"][k], 1 if k == "own" else k
        assert (out["info"] == 0).all(), (k, out["info"])
        assert out["alpha"].shape == (3, kk, N) and out["cinv_diag"].shape == (3, N) and out["cov_diag"].shape == (3, N)
        assert out["comp"].shape == (3, 3 + nl, kk, N) and out["flux"].shape == (3, N)
        assert all(np.isfinite(out[key]).all() for key in ALL)
        np.testing.assert_array_equal(out["flux"], c["tr"]["flux"])
    # how the right-hand sides were cut: 48 rows in all below 113 pixels, 32 up to 128, 16 up to 144
    rows_in_all = 48 if c["W"] <= 112 else 32 if c["W"] <= 128 else 16
    assert c["kmax"] == rows_in_all - m
    if name == "N330-narrow":
        assert D.rhs_groups(30, c["kmax"]) == [(0, 30)] and m + 30 > 32      # one call, three blocks of right-hand sides
    if name == "N256":
        assert D.rhs_groups(30, c["kmax"]) == [(0, 28), (28, 30)]            # one Python-level call, two groups
    if name == "N180-m17":
        assert D.rhs_groups(13, c["kmax"]) == [(0, 13)] and D.rhs_groups(30, c["kmax"]) == [(0, 15), (15, 30)]
    assert do.diagnose_banded_max_nrhs(145) == 0 and do.diagnose_banded_max_nrhs(0) == 48 - m


@pytest.mark.parametrize("name", CASES)
def test_alpha_solves_the_oracles_system(name):
    c = case(name)
    N = c["N"]
    fac = 1e-13 + N * gamma(3 * N + 1)
    worst = {"band": 0.0, "dense": 0.0}
    for b in range(3):
        ref = reference(c, b)
        C = ref["C"]
        cnorm = np.abs(C).sum(axis=1).max()
        amp = BR.amplification(ref["Bd"], ref["Y"])
        for k in KS:
            R = rhs_rows(c, k, b)
            for which, out in (("band", c["band"][k]), ("dense", c["pointwise"].get(k))):
                if out is None:
                    continue
                x = out["alpha"][b]
                lhs = np.abs(x @ C - R).max(axis=1)
                rhs = fac * (cnorm * np.abs(x).max(axis=1) + np.abs(R).max(axis=1))
                ratio = float((lhs / rhs).max())
                worst[which] = max(worst[which], ratio)
                print(f"{name} walker {b} k={k} {which}: max |C x - R|_inf / bound = {ratio:.3g} "
                      f"(||Bd^-1|| ||Y^T Y|| = {amp:.3g}, ||C|| = {cnorm:.3g})")
                if which == "band":
                    assert ratio <= 1.0, (name, b, k, ratio)
    print(f"{name}: largest |C x - R|_inf / bound: band {worst['band']:.3g}, dense {worst['dense']:.3g}")


@pytest.mark.parametrize("name", CASES)
def test_cov_diag_is_the_diagonal_that_is_factorised(name):
    c = case(name)
    for b, p in enumerate(c["plist"]):
        ref = np.diag(O.forward_model(c["oo"], p)[1]) + 1e-10
        for k in KS:
            got = c["band"][k]["cov_diag"][b]
            print(f"{name} walker {b} k={k}: max rel |cov_diag - oracle| = {np.abs(got / ref - 1).max():.3g}")
            np.testing.assert_allclose(got, ref, rtol=1e-13, atol=0)


@pytest.mark.parametrize("name", CASES)
def test_cinv_diag_within_the_bound_of_the_longdouble_inverse(name):
    c = case(name)
    npad, m, W = c["do"].npad, c["m"], c["W"]
    for b in range(3):
        ref = reference(c, b)
        L64, X64 = ref["L"].astype(np.float64), ref["X"].astype(np.float64)  # (the reference factor rounded to float64)
        aL, aCi = np.abs(L64), np.abs(X64.T @ X64)
        b1 = first_bound(L64, X64, npad).astype(np.float64)
        dC = 1e-13 * np.abs(ref["C"]) + gamma(npad + 1) * (aL @ aL.T)
        b2 = np.sum((aCi @ dC) * aCi, axis=1) + b1
        sel = SR.selinv_bound(ref["Bd"], W, ref["LB"])[:, 0]
        cancel = gamma(m + 1) * (ref["sigma_diag"] + np.sum(ref["Vs"] * ref["Vs"], axis=1)).astype(np.float64)
        bound = b2 + sel + cancel
        d = ref["cinv_diag"]
        fracs = {}
        for which, out in (("band", c["band"]["own"]), ("dense", c["pointwise"]["own"])):
            err = np.abs(out["cinv_diag"][b].astype(LD) - d).astype(np.float64)
            fracs[which] = float((err / bound).max())
            ratio = out["cov_diag"][b] * out["cinv_diag"][b]
            print(f"{name} walker {b} {which}: max err / bound = {fracs[which]:.3g} (against bound (2) alone "
                  f"{float((err / b2).max()):.3g}), max rel err = {float((err / d.astype(np.float64)).max()):.3g}; "
                  f"diag(C) diag(C^-1) in [{ratio.min():.6g}, {ratio.max():.3g}]")
        apart = np.abs(c["band"]["own"]["cinv_diag"][b] / c["pointwise"]["own"]["cinv_diag"][b] - 1).max()
        print(f"{name} walker {b}: band against dense, max rel difference = {apart:.3g}")
        assert fracs["band"] <= 1.0, (name, b, fracs)
        assert (c["band"]["own"]["cov_diag"][b] * c["band"]["own"]["cinv_diag"][b] >= 1 - 1e-12).all()
        # the reference's own identity: diag(Sigma) - rowsum(Vs^2) is the diagonal of the inverse
        own = BR.cinv_diag(ref["sigma_diag"], ref["Vs"])
        assert float(np.abs(own / d - 1).max()) <= 1e-12


@pytest.mark.parametrize("name", CASES)
def test_components_are_the_oracles_kernels_times_alpha_and_add_up(name):
    c = case(name)
    wave, m = c["oo"].wave, c["m"]
    s2 = c["oo"].sigma.astype(LD) ** 2 + LD(1e-10)
    worst = [0.0, 0.0, 0.0]
    for b, p in enumerate(c["plist"]):
        for k in KS:
            out = c["band"][k]
            for j in range(out["alpha"].shape[1]):
                comp, alpha = out["comp"][b, :, j], out["alpha"][b, j]
                r = structured_ratios(wave, p, comp, alpha)
                assert max(r) <= 1.0, (name, b, k, j, r)
                if "global_cov" not in p:
                    assert (comp[2] == 0).all()
                want = s2 * alpha.astype(LD)
                rel = float((np.abs(comp[1].astype(LD) - want) / np.abs(want)).max())
                assert rel <= 2 * U, (name, b, k, j, rel)
                total, _ = sum_ratio(c["cov"][b], m, comp, alpha)
                assert total <= 1.0, (name, b, k, j, total)
                worst = [max(worst[0], max(r)), max(worst[1], rel / U), max(worst[2], total)]
    print(f"{name}: largest ratio to the bound: structured {worst[0]:.3g}, noise {worst[1]:.3g} u, sum identity {worst[2]:.3g}")
    # the dense call through the same check (printed: the yardstick)
    for b, p in enumerate(c["plist"]):
        out = c["decompose"][2]
        r = [max(structured_ratios(wave, p, out["comp"][b, :, j], out["alpha"][b, j])) for j in range(2)]
        print(f"{name} walker {b} dense: structured {max(r):.3g}")


@pytest.mark.parametrize("name", CASES)
def test_repeated_chunked_and_sub_batch_calls_give_the_same_bits(name):
    c = case(name)
    do, md, rows, W = c["do"], c["md"], c["rows"], c["W"]
    for k in ("own", 13, 30) if name in ("N256", "N330-narrow") else (2,):
        rhs, want = c["rhs"][k], c["band"][k]
        for other in (do.diagnose_banded(md, rows, rhs, want=ALL, want_flux=True),
                      do.diagnose_banded(md, rows, rhs, want=ALL, want_flux=True, max_chunk=2)):
            for key in ALL + ("info", "flux"):
                np.testing.assert_array_equal(other[key], want[key], err_msg=f"{k} {key}")
        # walkers 0 and 2 alone, at the half-width of the whole group
        sub = None if rhs is None else (rhs[[0, 2]] if rhs.ndim == 3 else rhs)
        pieces = []
        with D._torch().cuda.device(do.dev):
            R, nrhs, per_walker = do._rhs_on_device(sub, 2)
            for cols in D.rhs_groups(nrhs, c["kmax"]):
                pieces.append(do._diagnose_banded_group(md, rows[[0, 2]], W, R, per_walker, cols, ALL, False, None))
        np.testing.assert_array_equal(np.concatenate([q["alpha"] for q in pieces], axis=1), want["alpha"][[0, 2]])
        np.testing.assert_array_equal(np.concatenate([q["comp"] for q in pieces], axis=2), want["comp"][[0, 2]])
        for q in pieces:
            np.testing.assert_array_equal(q["cinv_diag"], want["cinv_diag"][[0, 2]])
            np.testing.assert_array_equal(q["cov_diag"], want["cov_diag"][[0, 2]])
            assert (q["info"] == 0).all()
    # the two diagonals do not depend on the right-hand sides: not on their values, their number or their blocks
    for k in KS[1:]:
        np.testing.assert_array_equal(c["band"][k]["cinv_diag"], c["band"]["own"]["cinv_diag"], err_msg=str(k))
        np.testing.assert_array_equal(c["band"][k]["cov_diag"], c["band"]["own"]["cov_diag"], err_msg=str(k))
    # asking for less gives the same alpha, and the three dense-style entry points are this call
    only = do.diagnose_banded(md, rows, c["rhs"][2])
    assert set(only) == {"alpha", "info"}
    np.testing.assert_array_equal(only["alpha"], c["band"][2]["alpha"])
    ap, pw, de = (do.apply(md, rows, "Cinv", c["rhs"][2], solver="banded"), do.pointwise(md, rows, c["rhs"][2], solver="auto"),
                  do.decompose(md, rows, c["rhs"][2], solver="banded"))
    assert set(ap) == {"out", "info"} and set(pw) == {"alpha", "cinv_diag", "cov_diag", "info"} and set(de) == {"alpha", "comp", "info"}
    np.testing.assert_array_equal(ap["out"], c["band"][2]["alpha"])
    for key in ("alpha", "cinv_diag", "cov_diag"):
        np.testing.assert_array_equal(pw[key], c["band"][2][key], err_msg=key)
    for key in ("alpha", "comp"):
        np.testing.assert_array_equal(de[key], c["band"][2][key], err_msg=key)
    # the dense calls keep their bits beside the new one
    np.testing.assert_array_equal(do.pointwise(md, rows, c["rhs"][2])["cinv_diag"], c["pointwise"][2]["cinv_diag"])


def keys_of(model):
    return (len(model.residuals), model._lnprob, model._log_scale, model._glob_snapshot, model._loc_snapshot)


def test_model_methods_take_the_solver_and_default_to_the_dense_bits():
    c = case("N256")
    N, P = c["N"], c["P"]
    rhs = c["rhs"][2]
    for built_with in ("dense", "auto"):
        model = synth.build_model(c["o"], solver=built_with)
        l0 = model.log_likelihood()
        before = keys_of(model)
        dev, md, rows = model._pack(P, update_caches=False)
        # solver=None: bit for bit what the methods give today, from the DeviceOrder dense calls
        raw_p, raw_d, raw_a = dev.pointwise(md, rows, rhs), dev.decompose(md, rows, rhs), dev.apply(md, rows, "Cinv", rhs)
        for solver in (None, "dense"):
            got, info = model.pointwise_batch(P, rhs, return_info=True, solver=solver)
            want = model._pointwise_dict(rhs, raw_p["alpha"], raw_p["cinv_diag"], raw_p["cov_diag"], False)
            assert (info == 0).all()
            for key in want:
                np.testing.assert_array_equal(got[key], want[key], err_msg=key)
            got = model.residual_components_batch(P, rhs, solver=solver)
            want = model._component_dict(raw_d["comp"], raw_d["alpha"], True, 1, False)
            for key in want:
                np.testing.assert_array_equal(got[key], want[key], err_msg=key)
            np.testing.assert_array_equal(model.apply_factor_batch(P, "Cinv", rhs, solver=solver), raw_a["out"])
        # the band solver: what DeviceOrder.diagnose_banded gives, which is not the dense call's bits
        band = dev.diagnose_banded(md, rows, rhs, want=ALL, solver="auto")
        assert (band["info"] == 0).all() and (dev.halfwidth_bound(md, rows) <= dev.banded_window_halfwidth()).all()
        for solver in ("banded", "auto"):
            got, info = model.pointwise_batch(P, rhs, return_info=True, solver=solver)
            want = model._pointwise_dict(rhs, band["alpha"], band["cinv_diag"], band["cov_diag"], False)
            assert (info == 0).all()
            for key in want:
                np.testing.assert_array_equal(got[key], want[key], err_msg=key)
            got = model.residual_components_batch(P, rhs, solver=solver)
            want = model._component_dict(band["comp"], band["alpha"], True, 1, False)
            for key in want:
                np.testing.assert_array_equal(got[key], want[key], err_msg=key)
            np.testing.assert_array_equal(model.apply_factor_batch(P, "Cinv", rhs, solver=solver), band["alpha"])
        assert not np.array_equal(band["alpha"], raw_a["out"])  # (another solve: agreement to rounding, not bit for bit)
        np.testing.assert_allclose(band["alpha"], raw_a["out"], rtol=0, atol=1e-9 * np.abs(raw_a["out"]).max())
        # own residual, batch and scalar
        own = dev.diagnose_banded(md, rows, None, want=ALL, want_flux=True)
        got = model.pointwise_batch(P, solver="banded")
        want = model._pointwise_dict((own["flux"] - model.data.flux)[:, None, :], own["alpha"], own["cinv_diag"], own["cov_diag"], True)
        for key in want:
            np.testing.assert_array_equal(got[key], want[key], err_msg=key)
        dev, md1, row1 = model._pack(update_caches=False)  # the model's own state
        one = dev.diagnose_banded(md1, row1, None, want=ALL, want_flux=True)
        assert (one["info"] == 0).all()
        np.testing.assert_array_equal(model.cho_solve(solver="banded"), one["alpha"][0, 0])
        np.testing.assert_array_equal(model.cho_solve(rhs[0], solver="auto"), dev.diagnose_banded(md1, row1, rhs[0])["alpha"][0])
        np.testing.assert_array_equal(model.pointwise(solver="auto")["alpha"], one["alpha"][0, 0])
        np.testing.assert_array_equal(model.pointwise(solver="auto")["loo_std"], 1.0 / np.sqrt(one["cinv_diag"][0]))
        comps = model.residual_components(solver="banded")
        np.testing.assert_array_equal(comps["global"], one["comp"][0, 2, 0])
        np.testing.assert_array_equal(comps["local"], one["comp"][0, 3:, 0])
        total = comps["emulator"] + comps["noise"] + comps["global"] + comps["local"].sum(axis=0)
        resid = one["flux"][0] - model.data.flux
        assert np.abs(total - resid).max() <= 1e-9 * np.abs(resid).max()
        # whiten and draw stay on the dense factor; no method disturbs the model's state
        assert model.whiten().shape == (N,) and model.draw(rng=1).shape == (N,)
        with pytest.raises(ValueError, match="Cinv"):
            model.apply_factor_batch(P, "Linv", solver="banded")
        with pytest.raises(ValueError, match="triangular factor"):
            dev.apply(md, rows, "L", solver="auto")
        assert keys_of(model) == before
        assert model.log_likelihood() == l0


def test_failed_walkers_get_nan_rows_and_leave_the_others_alone():
    """The mixed batch of tests/test_gpu_pointwise.py (data without pixel noise; log_scale 18, which the dense factorisation
    finds not positive definite; T = 1e5, outside the grid) and one walker whose global length scale puts its bound beyond
    the window."""
    N = 256
    o = dict(synth.make_order(N=N, m=4, seed=5))
    o["sigma"] = np.zeros(N)
    model = synth.build_model(o)
    P = synth.walker_ball(o, B=3, seed=21)
    not_pd, off_grid, wide = P[1].copy(), P[2].copy(), P[0].copy()
    not_pd[2] = 18.0
    off_grid[synth.LABELS.index("T")] = 1e5
    wide[synth.LABELS.index("global_cov:log_ls")] = float(np.log(14.0))
    mixed = np.stack([P[0], not_pd, P[1], off_grid, P[2], wide])
    dev, md, rows = model._pack(mixed, update_caches=False)
    hw, window = dev.halfwidth_bound(md, rows), dev.banded_window_halfwidth()
    print("half-width bounds", hw, "window", window)
    assert hw[5] > window and (hw[:5] <= window).all() and hw[:5].max() == hw[[0, 2, 4]].max()
    rhs = np.random.default_rng(2).standard_normal((2, N))
    keys = ("alpha", "marginal_std", "loo_mean", "loo_std", "z", "log_density")
    for r in (None, rhs):
        good, info0 = model.pointwise_batch(P, r, return_info=True, solver="banded")
        assert (info0 == 0).all() and all(np.isfinite(v).all() for v in good.values())
        got, info = model.pointwise_batch(mixed, r, return_info=True, solver="banded")
        print("info under banded", info)
        assert info[3] == -1 and info[5] == D.INFO_BANDWIDTH and (info[[0, 2, 4]] == 0).all(), info
        for key in keys:
            for b in (1, 3, 5):  # (the band solver factorises Bd, not C: it may well take the walker the dense call refuses)
                assert np.isnan(got[key][b]).all() == (info[b] != 0), (key, b)
            assert np.isnan(got[key][3]).all() and np.isnan(got[key][5]).all(), key
            np.testing.assert_array_equal(got[key][[0, 2, 4]], good[key], err_msg=key)
        comps, cinfo = model.residual_components_batch(mixed, r, return_info=True, solver="banded")
        np.testing.assert_array_equal(cinfo, info)
        gcomps = model.residual_components_batch(P, r, solver="banded")
        for key in comps:
            assert np.isnan(comps[key][3]).all() and np.isnan(comps[key][5]).all(), key
            np.testing.assert_array_equal(comps[key][[0, 2, 4]], gcomps[key], err_msg=key)
        # "auto": the wide walker is the dense call's, bit for bit; the others keep the band solver's bits
        auto, ainfo = model.pointwise_batch(mixed, r, return_info=True, solver="auto")
        dense, dinfo = model.pointwise_batch(mixed[5:], r, return_info=True)
        assert ainfo[5] == 0 and dinfo[0] == 0 and ainfo[3] == -1
        for key in keys:
            np.testing.assert_array_equal(auto[key][5], dense[key][0], err_msg=key)
            np.testing.assert_array_equal(auto[key][[0, 2, 4]], good[key], err_msg=key)
        acomps = model.residual_components_batch(mixed, r, solver="auto")
        dcomps = model.residual_components_batch(mixed[5:], r)
        for key in acomps:
            np.testing.assert_array_equal(acomps[key][5], dcomps[key][0], err_msg=key)
        solved = model.apply_factor_batch(mixed, "Cinv", r, solver="auto")
        np.testing.assert_array_equal(solved[5], model.apply_factor_batch(mixed[5:], "Cinv", r)[0])
    raw = dev.diagnose_banded(md, rows, rhs, want=ALL, want_flux=True)
    for key in ALL:
        assert np.isnan(raw[key][[3, 5]]).all() and np.isfinite(raw[key][[0, 2, 4]]).all(), key
    # the scalar methods raise as log_likelihood does
    model.set_param_vector(off_grid)
    for call in (model.pointwise, model.cho_solve, model.residual_components):
        for solver in ("banded", "auto"):
            with pytest.raises(ValueError, match="emulator"):
                call(solver=solver)
    model.set_param_vector(wide)
    with pytest.raises(ValueError, match="band"):
        model.pointwise(solver="banded")
    assert np.isfinite(model.pointwise(solver="auto")["z"]).all()


# ------------------------------------------------------------------------------------------ the C-ABI call itself
def raw_call(do, md, rows, W, rhs=None, ldr=None, want=(True, True, True), guard=32, B=None, nrhs=None, rhs_stride=None,
             null=(), ws_bytes=None, ctx=None, check=True):
    """sf_diagnose_banded_batch called directly.  rhs: None or (B, k, n) / (k, n), laid out with row stride ``ldr`` >= n and
    NaN behind row n of each; ``guard`` sentinel doubles behind every output.  Returns the return code, the outputs without
    and the guards, info."""
    import torch

    n = do.n
    Bt = rows.shape[0]
    B = Bt if B is None else B
    ncomp = 3 + int(md.n_local)
    with torch.cuda.device(do.dev):
        P = D.to_dev(rows, do.dev)
        R, k, stride = None, 1, 0
        if rhs is not None:
            k = rhs.shape[-2]
            ldr = ldr or n
            ld = max(ldr, n)  # (a refused ldr < n is handed over, not laid out)
            padded = np.full(rhs.shape[:-1] + (ld,), np.nan)
            padded[..., :n] = rhs
            R = D.to_dev(padded, do.dev)
            stride = k * ld if rhs.ndim == 3 else 0
        k = k if nrhs is None else nrhs
        stride = stride if rhs_stride is None else rhs_stride
        kk = max(k, 1)
        sizes = dict(alpha=Bt * kk * n, cinv_diag=Bt * n, cov_diag=Bt * n, comp=Bt * ncomp * kk * n)
        wanted = dict(alpha=True, cinv_diag=want[0], cov_diag=want[1], comp=want[2])
        bufs = {key: torch.full((sizes[key] + guard,), SENTINEL, dtype=torch.float64, device=do.dev) if wanted[key] else None
                for key in sizes}
        info = torch.full((Bt,), 77, dtype=torch.int32, device=do.dev)
        need = do.diagnose_banded_workspace_bytes(md, max(min(B, Bt), 1), W, kk, want[0], want[2])
        ws = D.empty((max(need if ws_bytes is None else ws_bytes, 256),), do.dev, torch.uint8)
        args = dict(params=D.ptr(P), alpha=D.ptr(bufs["alpha"]), work=D.ptr(ws))
        for key in null:
            args[key] = D.ptr(None)
        rc = do.lib.sf_diagnose_banded_batch(do.ctx if ctx is None else ctx, _lib.C.byref(md), B, args["params"], W, D.ptr(R), k,
                                             ldr or n, stride, args["alpha"], D.ptr(bufs["cinv_diag"]), D.ptr(bufs["cov_diag"]),
                                             D.ptr(bufs["comp"]), D.ptr(None), D.ptr(info), args["work"],
                                             ws.numel() if ws_bytes is None else ws_bytes, D.stream_ptr(do.dev))
        if check:
            _lib.check(rc, "sf_diagnose_banded_batch")
        torch.cuda.synchronize(do.dev)
        host = {key: (None if t is None else t.cpu().numpy()) for key, t in bufs.items()}
        shapes = dict(alpha=(Bt, kk, n), cinv_diag=(Bt, n), cov_diag=(Bt, n), comp=(Bt, ncomp, kk, n))
        outs = {key: (None if v is None else v[:-guard].reshape(shapes[key])) for key, v in host.items()}
        guards = {key: (None if v is None else v[-guard:]) for key, v in host.items()}
        return rc, outs, guards, info.cpu().numpy()


def test_padding_of_the_inputs_is_not_read_and_nothing_is_written_behind_the_outputs():
    c = case("N180")
    do, md, rows, W = c["do"], c["md"], c["rows"], c["W"]
    for k, ldr in ((2, 187), (13, 181)):
        rhs, want = c["rhs"][k], c["band"][k]
        rc, outs, guards, info = raw_call(do, md, rows, W, rhs, ldr=ldr)
        assert rc == 0 and (info == 0).all()
        for key in ALL:
            np.testing.assert_array_equal(outs[key], want[key], err_msg=key)
            assert (guards[key] == SENTINEL).all(), key
    # the own residual; and a NULL output is not computed, the others keep their bits
    rc, outs, guards, info = raw_call(do, md, rows, W)
    for key in ALL:
        np.testing.assert_array_equal(outs[key], c["band"]["own"][key], err_msg=key)
        assert (guards[key] == SENTINEL).all(), key
    for want in ((False, False, False), (True, False, False), (False, True, True)):
        rc, outs, guards, info = raw_call(do, md, rows, W, c["rhs"][2], want=want)
        assert rc == 0 and (info == 0).all()
        for key, asked in zip(ALL, (True,) + want):
            assert (outs[key] is None) == (not asked)
            if asked:
                np.testing.assert_array_equal(outs[key], c["band"][2][key], err_msg=key)
                assert (guards[key] == SENTINEL).all(), key


def test_workspace_grows_and_every_refusal_enqueues_nothing():
    c = case("N180")
    do, md, rows, W, n, m = c["do"], c["md"], c["rows"], c["W"], c["N"], c["m"]
    q = do.diagnose_banded_workspace_bytes
    sizes = np.array([[q(md, B, W, k) for k in (1, 2, 12, 13, 28)] for B in (1, 2, 3, 64)])
    assert (sizes > 0).all() and (np.diff(sizes, axis=0) > 0).all() and (np.diff(sizes, axis=1) > 0).all()
    for B, k in ((1, 1), (3, 13)):
        assert q(md, B, W, k, True, False) > q(md, B, W, k) and q(md, B, W, k, False, True) > q(md, B, W, k)
        assert q(md, B, W, k, True, True) > max(q(md, B, W, k, True, False), q(md, B, W, k, False, True))
    kmax = c["kmax"]
    assert kmax == 32 - m and q(md, 3, W, kmax) > 0
    perm = np.random.default_rng(12).permutation(n)
    oo = c["oo"]
    shuffled = D.DeviceOrder(oo.wave[perm], oo.flux[perm], oo.sigma[perm], oo.min_dv_wave, oo.bulk_fluxes, oo.grid_points,
                             oo.variances, oo.lengthscales, oo.v11, oo.w_hat)
    assert shuffled.diagnose_banded_max_nrhs(W) == 0 and do.lib.sf_diagnose_banded_max_nrhs(None, W) == -1
    bad_md = do.model_desc(1, 1, 1, 1, 1, 2)
    bad_md.n_local = -1
    # the size query returns 0 for whatever the call refuses
    for B, w, k in ((0, W, 1), (65536, W, 1), (3, W, 0), (3, W, kmax + 1), (3, -1, 1), (3, 145, 1), (3, 129, 16 - m + 1)):
        assert q(md, B, w, k) == 0, (B, w, k)
    assert shuffled.diagnose_banded_workspace_bytes(md, 3, W, 1) == 0 and q(bad_md, 3, W, 1) == 0
    assert do.lib.sf_diagnose_banded_workspace_bytes(None, _lib.C.byref(md), 3, W, 1, 0, 0) == 0
    rhs = c["rhs"][2]
    refusals = [
        (dict(B=0), "1 .. 65535"), (dict(B=65536), "1 .. 65535"), (dict(rhs=rhs, nrhs=0), "positive"),
        (dict(rhs=np.zeros((kmax + 1, n))), "sf_diagnose_banded_max_nrhs.*sf_pointwise_batch"),
        (dict(null=("params",)), "required"), (dict(null=("alpha",)), "required"), (dict(null=("work",)), "required"),
        (dict(rhs=rhs, rhs_stride=-1), "rhs_stride"), (dict(nrhs=2), "nrhs == 1 without"), (dict(rhs=rhs, ldr=n - 1), "ldr"),
        (dict(do=shuffled), "strictly increasing"), (dict(ctx=_lib.C.c_void_p(0)), "context"), (dict(md=bad_md), "model"),
        (dict(W=145), "sf_pointwise_batch"),
    ]
    import re

    for kw, message in refusals:
        kw = dict(kw)
        rc, outs, guards, info = raw_call(kw.pop("do", do), kw.pop("md", md), rows, kw.pop("W", W), check=False, **kw)
        said = do.lib.sf_last_error().decode()
        assert rc == -1 and re.search(message, said), (kw, rc, said)
        assert (info == 77).all() and all((v == SENTINEL).all() for v in outs.values() if v is not None), (kw, said)
    rc, outs, guards, info = raw_call(do, md, rows, W, rhs, ws_bytes=q(md, 3, W, 2, True, True) - 256, check=False)
    assert rc == -2 and "workspace too small" in do.lib.sf_last_error().decode()
    assert (info == 77).all() and all((v == SENTINEL).all() for v in outs.values())
    # a half-width below a walker's support flags it: SF_INFO_BANDWIDTH and NaN rows
    rc, outs, guards, info = raw_call(do, md, rows, 16, rhs)
    assert rc == 0 and (info == D.INFO_BANDWIDTH).all() and all(np.isnan(v).all() for v in outs.values())
