"""sf_decompose_batch through DeviceOrder.decompose: alpha = C^-1 rhs and the conditional means K_k alpha of the covariance
components (0 emulator, 1 noise + jitter, 2 global, 3 + j local kernel j), which add up to rhs.

Orders: N = 180 (npad 192 = 64 mod 128: the factorisation's shifted frame, and a partial last 64-row block) and N = 256,
three walkers with different parameters.  Bounds: u = 2^-53, gamma_k = k u / (1 - k u) for a sum of k terms (Higham,
Accuracy and Stability of Numerical Algorithms, section 3.1), plus the project's 1e-13 element contract of the covariance
fill (SURVEY 8 d), whose element formulas the kernel evaluates.  Every check takes alpha from the call's own output, in long
double: it tests the products, not the solve (tests/test_gpu_apply_factor.py does that)."""
import numpy as np
import pytest

from oracle import sf_oracle as O
from starfish_amd import _device as D
from starfish_amd import synth

from gpu_helpers import device_order, oracle_order, pack_rows

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble


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
        c["dec"] = do.decompose(md, rows, want_flux=True)
        assert (c["dec"]["info"] == 0).all()
        c["cov"] = do.forward(md, rows)["cov"]
        _CASES[N] = c
    return _CASES[N]


def ratio_to_bound(got, K, alpha, fac):
    """max over the rows of |got - K alpha| / (fac |K| |alpha|), in long double; a row whose bound is zero must be exact."""
    K, a = np.asarray(K).astype(LD), np.asarray(alpha).astype(LD)
    err, bound = np.abs(np.asarray(got).astype(LD) - K @ a), LD(fac) * (np.abs(K) @ np.abs(a))
    assert (err[bound == 0] == 0).all()
    return float(np.max(err[bound > 0] / bound[bound > 0])) if (bound > 0).any() else 0.0


def structured_ratios(wave, p, comp, alpha):
    """The ratios of ratio_to_bound for the global and every local component of one walker and one right-hand side
    (comp: (ncomp, n)) against the oracle's matrices, bound factor 1e-13 + gamma_{n+2}."""
    n = len(wave)
    fac = 1e-13 + gamma(n + 2)
    out = []
    if "global_cov" in p:
        la, ll = p["global_cov"]
        out.append(ratio_to_bound(comp[2], O.matern32_global(wave, np.exp(la), np.exp(ll)), alpha, fac))
    for j, (mu, la, ls) in enumerate(p.get("local_cov", [])):
        out.append(ratio_to_bound(comp[3 + j], O.gaussian_local(wave, np.exp(la), mu, np.exp(ls)), alpha, fac))
    return out


def sum_ratio(cov, m, comp, alpha):
    """|sum_k comp_k - (C_dev + 1e-10 I) alpha| against (1e-13 + gamma_{n+m+4}) |C_dev| |alpha| (comp: (ncomp, n))."""
    n = cov.shape[0]
    Cj = cov.astype(LD) + LD(1e-10) * np.eye(n, dtype=LD)
    a = alpha.astype(LD)
    err = np.abs(comp.astype(LD).sum(axis=0) - Cj @ a)
    bound = LD(1e-13 + gamma(n + m + 4)) * (np.abs(cov.astype(LD)) @ np.abs(a))
    return float(np.max(err / bound)), bound


@pytest.mark.parametrize("N", [180, 256])
def test_structured_components_are_the_oracles_kernels_times_alpha(N):
    c = case(N)
    out = c["dec"]
    assert out["comp"].shape == (3, 4, 1, N) and out["alpha"].shape == (3, 1, N)
    for b, p in enumerate(c["plist"]):
        r = structured_ratios(c["oo"].wave, p, out["comp"][b, :, 0], out["alpha"][b, 0])
        print(f"N={N} walker {b}: |comp - K alpha| / bound: global {r[0]:.3g}, local {r[1]:.3g}")
        assert max(r) <= 1.0
        assert np.abs(out["comp"][b, 2:, 0]).max() > 0


@pytest.mark.parametrize("N", [180, 256])
def test_noise_component_is_the_jittered_variance_times_alpha(N):
    c = case(N)
    s2 = c["oo"].sigma.astype(LD) ** 2 + LD(1e-10)
    for b in range(3):
        want = s2 * c["dec"]["alpha"][b, 0].astype(LD)
        rel = np.abs(c["dec"]["comp"][b, 1, 0].astype(LD) - want) / np.abs(want)
        print(f"N={N} walker {b}: noise component, max relative error {float(rel.max() / U):.3g} u")
        assert (rel <= 2 * U).all()


@pytest.mark.parametrize("N", [180, 256])
def test_components_add_up_to_the_covariance_times_alpha_and_to_the_residual(N):
    """The sum identity pins the emulator component: C_dev is the matrix sf_forward_batch fills (no jitter).  Against the
    residual: the bound of test_cinv_of_the_residual_solves_the_oracles_system (tests/test_gpu_apply_factor.py) for
    |C alpha - r|, plus the matvec term."""
    c = case(N)
    out, m = c["dec"], c["do"].m
    np.testing.assert_array_equal(out["flux"], c["tr"]["flux"])
    fac = 1e-13 + N * gamma(3 * N + 1)
    for b, p in enumerate(c["plist"]):
        comp, alpha, R = out["comp"][b, :, 0], out["alpha"][b, 0], c["tr"]["resid"][b]
        ratio, mv = sum_ratio(c["cov"][b], m, comp, alpha)
        C_ref = O.forward_model(c["oo"], p)[1] + 1e-10 * np.eye(N)
        lhs = float(np.abs(comp.astype(LD).sum(axis=0) - R.astype(LD)).max())
        rhs = fac * (np.abs(C_ref).sum(axis=1).max() * np.abs(alpha).max() + np.abs(R).max()) + float(mv.max())
        print(f"N={N} walker {b}: |sum - (C + jitter) alpha| / bound = {ratio:.3g}; |sum - r|_inf = {lhs:.3g}, bound {rhs:.3g}")
        assert ratio <= 1.0
        assert lhs <= rhs


def test_alpha_is_apply_cinv_bit_for_bit_and_neither_call_disturbs_the_other():
    """Regression guard: loglike and apply("Cinv") return the same bits before and after a decompose call, and decompose's
    alpha is apply's result."""
    c = case(180)
    do, md, rows = c["do"], c["md"], c["rows"]
    ll0, ci0 = do.loglike(md, rows), do.apply(md, rows, "Cinv")
    dec = do.decompose(md, rows)
    ll1, ci1 = do.loglike(md, rows), do.apply(md, rows, "Cinv")
    for key in ("lnl", "logdet", "sqmah", "log_scale", "info"):
        np.testing.assert_array_equal(ll0[key], ll1[key])
    np.testing.assert_array_equal(ci0["out"], ci1["out"])
    np.testing.assert_array_equal(dec["alpha"], ci0["out"])
    for key in ("comp", "alpha", "info"):  # two identical calls give identical bits
        np.testing.assert_array_equal(dec[key], c["dec"][key])


def test_a_model_without_structured_kernels_has_three_components_and_a_zero_global_one():
    c = case(180)
    plist = [{k: v for k, v in p.items() if k not in ("global_cov", "local_cov")} for p in c["plist"]]
    md, rows = pack_rows(c["do"], plist)
    out = c["do"].decompose(md, rows)
    assert (out["info"] == 0).all() and out["comp"].shape == (3, 3, 1, 180)
    assert (out["comp"][:, 2] == 0).all()
    cov = c["do"].forward(md, rows)["cov"]
    for b in range(3):
        ratio, _ = sum_ratio(cov[b], c["do"].m, out["comp"][b, :, 0], out["alpha"][b, 0])
        print(f"no structured kernels, walker {b}: |sum - (C + jitter) alpha| / bound = {ratio:.3g}")
        assert ratio <= 1.0


def test_overlapping_local_kernels_and_one_outside_the_order():
    c = case(180)
    wave = c["oo"].wave
    plist = []
    for p in c["plist"]:
        mu, la, ls = p["local_cov"][0]
        plist.append(dict(p, local_cov=[(mu, la, ls), (mu * (1 + 20.0 / 2.99792458e5), la + 0.3, ls - 0.2),
                                        (wave[-1] * 1.01, la, ls)]))
    md, rows = pack_rows(c["do"], plist)
    out = c["do"].decompose(md, rows)
    assert (out["info"] == 0).all() and out["comp"].shape == (3, 6, 1, 180)
    assert (out["comp"][:, 5] == 0).all()  # 1 % = 3000 km/s beyond the last pixel, 4 sigma = 60 km/s
    cov = c["do"].forward(md, rows)["cov"]
    for b, p in enumerate(plist):
        r = structured_ratios(wave, p, out["comp"][b, :, 0], out["alpha"][b, 0])
        ratio, _ = sum_ratio(cov[b], c["do"].m, out["comp"][b, :, 0], out["alpha"][b, 0])
        print(f"three local kernels, walker {b}: ratios to the bound {np.round(r, 3)}, sum identity {ratio:.3g}")
        assert max(r) <= 1.0 and ratio <= 1.0
        assert np.abs(out["comp"][b, 3]).max() > 0 and np.abs(out["comp"][b, 4]).max() > 0


@pytest.mark.parametrize("nrhs", [1, 3, 17])
def test_right_hand_sides_across_the_group_of_16(nrhs):
    """17 crosses the 16-wide group.  Shared against per-walker right-hand sides: equal bits for equal vectors."""
    c = case(180)
    do, md, rows = c["do"], c["md"], c["rows"]
    rhs = np.random.default_rng(8).standard_normal((17, 180))[:nrhs]
    out = do.decompose(md, rows, rhs=rhs)
    assert (out["info"] == 0).all() and out["comp"].shape == (3, 4, nrhs, 180) and out["alpha"].shape == (3, nrhs, 180)
    worst, worst_sum = 0.0, 0.0
    for b, p in enumerate(c["plist"]):
        for r in range(nrhs):
            worst = max([worst] + structured_ratios(c["oo"].wave, p, out["comp"][b, :, r], out["alpha"][b, r]))
            worst_sum = max(worst_sum, sum_ratio(c["cov"][b], do.m, out["comp"][b, :, r], out["alpha"][b, r])[0])
    print(f"nrhs={nrhs}: largest ratio to the bound: structured {worst:.3g}, sum identity {worst_sum:.3g}")
    assert worst <= 1.0 and worst_sum <= 1.0
    per = do.decompose(md, rows, rhs=np.broadcast_to(rhs, (3,) + rhs.shape).copy())
    for key in ("comp", "alpha", "info"):
        np.testing.assert_array_equal(per[key], out[key])


def raw_decompose(do, md, rows, rhs, ldr, guard=64):
    """sf_decompose_batch called directly: per-walker right-hand sides (B, nrhs, n) laid out with row stride ``ldr`` > n and
    NaN behind row n of each; ``guard`` sentinel doubles behind comp and alpha.  Returns comp, alpha, info and the two
    guards as they come back."""
    import torch

    B, nrhs, n = rhs.shape
    ncomp = 3 + int(md.n_local)
    with torch.cuda.device(do.dev):
        P = D.to_dev(rows, do.dev)
        padded = np.full((B, nrhs, ldr), np.nan)
        padded[:, :, :n] = rhs
        R = D.to_dev(padded, do.dev)
        comp = torch.full((B * ncomp * nrhs * n + guard,), -7.0, dtype=torch.float64, device=do.dev)
        alpha = torch.full((B * nrhs * n + guard,), -7.0, dtype=torch.float64, device=do.dev)
        info = D.empty((B,), do.dev, torch.int32)
        ws = do._reserve(do.decompose_workspace_bytes(md, B, nrhs))
        do._call("decompose_batch", md, B, P, R, nrhs, ldr, nrhs * ldr, comp, alpha, None, info, ws=ws)
        comp, alpha = comp.cpu().numpy(), alpha.cpu().numpy()
        return (comp[:-guard].reshape(B, ncomp, nrhs, n), alpha[:-guard].reshape(B, nrhs, n), info.cpu().numpy(),
                comp[-guard:], alpha[-guard:])


def test_padding_of_the_inputs_is_not_read_and_nothing_is_written_behind_the_outputs():
    """N = 180 ends inside a 64-row block and inside a 256-column chunk.  The right-hand sides carry NaN behind row n; the
    outputs a guard behind their last row."""
    c = case(180)
    do, md, rows = c["do"], c["md"], c["rows"]
    rhs = np.random.default_rng(9).standard_normal((3, 2, 180))
    want = do.decompose(md, rows, rhs=rhs)
    comp, alpha, info, g_comp, g_alpha = raw_decompose(do, md, rows, rhs, ldr=187)
    assert (info == 0).all()
    np.testing.assert_array_equal(comp, want["comp"])
    np.testing.assert_array_equal(alpha, want["alpha"])
    assert (g_comp == -7.0).all() and (g_alpha == -7.0).all()
    a256 = lambda x: -(-x // 256) * 256  # noqa: E731
    for B, k in ((3, 2), (1, 1), (64, 17)):  # behind sf_apply_batch's layout: t = Y alpha, m doubles per right-hand side
        assert do.decompose_workspace_bytes(md, B, k) - do.apply_workspace_bytes(md, B, k) == a256(8 * B * k * do.m), (B, k)
    assert do.decompose_workspace_bytes(md, 0, 1) == 0 and do.decompose_workspace_bytes(md, 1, 0) == 0


def test_a_walker_outside_the_grid_gets_nan_rows_and_leaves_its_neighbours_alone():
    c = case(180)
    do, md = c["do"], c["md"]
    off = dict(c["plist"][1], grid=[1e5] + list(c["plist"][1]["grid"][1:]))
    _, mixed = pack_rows(do, [c["plist"][0], off, c["plist"][1], c["plist"][2]])
    out = do.decompose(md, mixed, want_flux=True)
    assert out["info"][1] == -1 and (out["info"][[0, 2, 3]] == 0).all()
    assert np.isnan(out["comp"][1]).all() and np.isnan(out["alpha"][1]).all()
    for key in ("comp", "alpha"):
        np.testing.assert_array_equal(out[key][[0, 2, 3]], c["dec"][key])
    chunked = do.decompose(md, mixed, want_flux=True, max_chunk=3)  # (chunks of 3 and 1 walkers)
    for key in ("comp", "alpha", "info"):
        np.testing.assert_array_equal(chunked[key], out[key])


def test_pixels_in_any_order_give_the_permuted_components():
    """A wavelength grid that is not monotonic: no column is culled.  The structured components of the permuted order are
    the permuted kernels times the call's alpha, within the bound of the sorted order."""
    c = case(180)
    oo = c["oo"]
    perm = np.random.default_rng(12).permutation(180)
    do = D.DeviceOrder(oo.wave[perm], oo.flux[perm], oo.sigma[perm], oo.min_dv_wave, oo.bulk_fluxes, oo.grid_points,
                       oo.variances, oo.lengthscales, oo.v11, oo.w_hat)
    out = do.decompose(c["md"], c["rows"])
    assert (out["info"] == 0).all()
    cov = do.forward(c["md"], c["rows"])["cov"]
    for b, p in enumerate(c["plist"]):
        r = structured_ratios(oo.wave[perm], p, out["comp"][b, :, 0], out["alpha"][b, 0])
        ratio, _ = sum_ratio(cov[b], do.m, out["comp"][b, :, 0], out["alpha"][b, 0])
        # (printed only: against the sorted order the difference is that of two solves of an ill-conditioned system)
        close = np.abs(out["comp"][b, :, 0] - c["dec"]["comp"][b, :, 0][:, perm]).max() / np.abs(c["dec"]["comp"][b]).max()
        print(f"permuted pixels, walker {b}: ratios to the bound {np.round(r, 3)}, sum identity {ratio:.3g}, "
              f"against the sorted order {close:.3g}")
        assert max(r) <= 1.0 and ratio <= 1.0
