"""sf_local_scan_batch through DeviceOrder.local_scan and the SpectrumModel methods: the score scan for a NEW local kernel of
centre mu and width sigma at amplitude 0, quad = alpha^T k alpha, trace = tr(W k), fisher = 1/2 tr(W k W k) with W = C^-1, alpha =
W r and k = the matrix the kernel adds at amplitude 1.

Orders: synth.make_order(N, m=4, seed=5) for N = 180 (npad 192: the factorisation's shifted frame, a partial last block) and N =
330, the three walkers of walker_ball(seed=3).  Models: "full" (global + one local kernel at N / 3: candidates overlap it),
"global" (global only) and "none" (no structured kernel at all).  Widths 8, 15 and 30 km/s at 2 km/s pixels: patches of up to 32,
60 and 120 pixels that lie inside one 64-block, straddle one boundary or span three blocks, clipped at both ends of the order.

The bound.  The device forms What = W + dW and alphahat = alpha + dalpha, the entries khat of k as the fill evaluates them, |khat -
k| <= 1e-13 k (the fill's entry contract), the products M = fl(What khat) and N = fl(khat What) and the three sums.  With u =
2^-53, gamma_K = K u / (1 - K u), to first order in dW, dalpha and u, against the longdouble reference of the oracle's matrix plus
jitter and the device's own residual (D = Dbar = k: every entry of k is >= 0):
  quad    2 |dalpha|^T k |alpha|                              + (1e-13 + 2 u + gamma_Kq) size_quad
  trace   sum |dW| o k                                        + (1e-13 +   u + gamma_Kq) size_trace
  fisher  1/2 sum (|dW| k |W| + |W| k |dW|) o k               + (2e-13 + 9 u + gamma_Kf) size_fisher
with |dW| the |dW| of tests/test_gpu_cov_fisher.py from the device's own factor L, X = L^-1: |dW| = |W| dC |W| + gamma_2n (E + E^T)
+ gamma_{n+1} |X|^T |X|, dC = 1e-13 |C| + gamma_{n+1} |L||L|^T, E = |X|^T |X||L||X|, n = npad; |dalpha| that of
tests/test_gpu_gradient.py: |W| dC |alpha| + |W| e (1e-13 + N gamma_{3N+1}) (|C|_inf |alpha|_inf + |r|_inf); the entry contract
once per k factor (one in quad and trace, two in fisher); u per product a thread forms (quad: alpha_a alpha_b, then times k;
trace: W k; fisher: three roundings for each of the products W k, k W and M o N, as tests/test_gpu_cov_fisher.py counts them).
The chains: a patch of at most 256 pixels spans nblk <= 5 blocks of 64, a thread adds its 16 entries of each of the npairs =
nblk (nblk + 1) / 2 block pairs, each pair's sum once more with its weight, then 6 shuffle steps and 3 adds over the waves: Kq = 17
npairs + 9 (264 at most); a tile of M and a tile of N sum at most 64 nblk products each: Kf = 128 nblk + Kq (904 at most).  The
matrix products of the bound itself are evaluated in float64.  A wrong-weight guard on top: every number agrees with the float64
numpy reference to 1e-6 size (a doubled diagonal pair or a dropped symmetric half is off by order 1e-1)."""
import ctypes

import numpy as np
import pytest

from oracle import sf_oracle as O
from starfish_amd import _device as D
from starfish_amd import _lib, synth

import local_scan_reference as LS
from gpu_helpers import device_order, oracle_order, pack_rows

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
SIGMAS = (8.0, 15.0, 30.0)
CASES = [f"N{N}-{kind}" for N in (180, 330) for kind in ("full", "global", "none")]
KEYS = ("quad", "trace", "fisher")


def gamma(k):
    return k * U / (1 - k * U)


def oracle_params(name, vec):
    p = synth.vector_to_oracle_params(vec)
    if not name.endswith("full"):
        del p["local_cov"]
    if name.endswith("none"):
        del p["global_cov"]
    return p


def candidates(wave):
    """Every pixel x the three widths (width-major), then the extra centres at 15 km/s: two between pixels (+0.3 and +0.5 of a
    step), one just outside the order whose patch is clipped, one far outside (no pixel in reach).  Returns the (ncand, 2) rows
    and the indices of the bound test's subset."""
    N = len(wave)
    step = wave[1] - wave[0]
    cand = [(w, s) for s in SIGMAS for w in wave]
    extra = [(wave[70] + 0.3 * step, 15.0), (wave[N // 2] + 0.5 * (wave[N // 2 + 1] - wave[N // 2]), 15.0), (wave[0] - 12 * step, 15.0),
             (wave[0] - 400 * step, 15.0)]
    pixels = sorted(set(range(0, N, 7)) | set(range(62, 67)) | set(range(126, 131)) | {0, 1, 2, N - 3, N - 2, N - 1})
    subset = [s * N + j for s in range(3) for j in pixels] + [3 * N + e for e in range(len(extra))]
    return np.array(cand + extra), np.array(subset)


_CASES = {}


def case(name):
    """Order, DeviceOrder, rows, candidates and the device results every test of that case shares (made once, never written)."""
    if name not in _CASES:
        N = int(name[1:4])
        o = synth.make_order(N=N, m=4, seed=5)
        oo = oracle_order(o)
        do = device_order(oo)
        P = synth.walker_ball(o, B=3, seed=3)
        plist = [oracle_params(name, p) for p in P]
        md, rows = pack_rows(do, plist)
        cand, subset = candidates(np.asarray(o["wave"]))
        c = dict(N=N, o=o, oo=oo, do=do, P=P, plist=plist, md=md, rows=rows, cand=cand, subset=subset)
        c["out"] = do.local_scan(md, rows, cand)
        c["resid"] = do.apply(md, rows, "Cinv", want_flux=True)["flux"] - oo.flux[None, :]
        c["C64"] = [O.forward_model(oo, p)[1] + O.JITTER * np.eye(N) for p in plist]
        _CASES[name] = c
    return _CASES[name]


def test_the_cases_cover_the_kernel_paths():
    """Patches inside one block, across one boundary, over three blocks, clipped at both ends, none at all; the model variants."""
    c = case("N330-full")
    lo, hi = D.local_scan_patches(c["o"]["wave"], c["cand"])
    nblk = hi // 64 - lo // 64 + 1
    width = hi - lo + 1
    assert set(np.unique(nblk[width > 0])) == {1, 2, 3} and width.max() <= 121 and (width[:-1] > 0).all() and width[-1] == 0
    assert lo.min() == 0 and hi.max() == 329 and width[3 * 330 + 2] < 30  # (clipped by the order's first pixel)
    assert (width[:330] < width[100]).sum() >= 10  # (8 km/s: the patches of the first and last pixels are clipped)
    assert case("N180-full")["do"].npad == 192 and c["do"].npad == 384
    kinds = {name: (bool(case(name)["md"].has_global), int(case(name)["md"].n_local)) for name in CASES[:3]}
    assert kinds == {"N180-full": (True, 1), "N180-global": (True, 0), "N180-none": (False, 0)}


@pytest.mark.parametrize("name", CASES)
def test_lnl_and_info_have_the_bits_of_loglike_and_every_number_is_finite(name):
    c = case(name)
    do, md, rows, out = c["do"], c["md"], c["rows"], c["out"]
    ll = do.loglike(md, rows)
    assert (ll["info"] == 0).all()
    np.testing.assert_array_equal(out["lnl"], ll["lnl"])
    np.testing.assert_array_equal(out["info"], ll["info"])
    for key in KEYS:
        assert out[key].shape == (3, len(c["cand"])) and np.isfinite(out[key]).all(), key


@pytest.mark.parametrize("name", CASES)
def test_the_subset_within_its_bound_of_the_longdouble_reference(name):
    c = case(name)
    do, md, rows, N, wave = c["do"], c["md"], c["rows"], c["N"], np.asarray(c["o"]["wave"])
    npad = do.npad
    fac = do.apply(md, rows, "L", rhs=np.eye(N))  # L e_j sums one product by 1 and zeros: the factor, exactly
    assert (fac["info"] == 0).all()
    Ldev = np.transpose(fac["out"], (0, 2, 1))
    worst = dict.fromkeys(KEYS, 0.0)
    for b in range(3):
        C64, r64 = c["C64"][b], c["resid"][b]
        W = LS.cinv(C64)
        alpha = W @ r64.astype(LD)
        W64 = LS.cinv(C64, np.float64)
        alpha64 = W64 @ r64
        # the pieces of the bound
        aL, aW, aal = np.abs(Ldev[b]), np.abs(W).astype(np.float64), np.abs(alpha).astype(np.float64)
        dC = 1e-13 * np.abs(C64) + gamma(npad + 1) * (aL @ aL.T)
        aX = np.abs(LS.inverse_longdouble(Ldev[b].astype(LD))).astype(np.float64)
        E = aX.T @ (aX @ (aL @ aX))
        dW = aW @ dC @ aW + gamma(2 * npad) * (E + E.T) + gamma(npad + 1) * (aX.T @ aX)
        solve = (1e-13 + N * gamma(3 * N + 1)) * (np.abs(C64).sum(axis=1).max() * aal.max() + np.abs(r64).max())
        d_alpha = aW @ (dC @ aal) + aW.sum(axis=1) * solve
        for q in c["subset"]:
            mu, sg = c["cand"][q]
            lo, hi, k = LS.patch_kernel(wave, mu, sg)
            got = [c["out"][key][b, q] for key in KEYS]
            if hi == lo:
                assert got == [0.0, 0.0, 0.0], (name, b, q, got)
                continue
            ref = LS.three(W, alpha, wave, mu, sg)
            ref64 = LS.three(W64, alpha64, wave, mu, sg)
            size = LS.sizes(W, alpha, wave, mu, sg)
            nblk = (hi - 1) // 64 - lo // 64 + 1
            Kq = 17 * (nblk * (nblk + 1) // 2) + 9
            Kf = 128 * nblk + Kq
            P = slice(lo, hi)
            first = (2 * d_alpha[P] @ k @ aal[P], np.sum(dW[P, P] * k),
                     0.5 * np.sum((dW[P, P] @ k @ aW[P, P] + aW[P, P] @ k @ dW[P, P]) * k))
            rel = (1e-13 + 2 * U + gamma(Kq), 1e-13 + U + gamma(Kq), 2e-13 + 9 * U + gamma(Kf))
            for key, g, rf, r64_, sz, f1, rl in zip(KEYS, got, ref, ref64, size, first, rel):
                bound = f1 + rl * sz
                err = abs(float(g - rf))
                worst[key] = max(worst[key], err / bound)
                assert err <= bound, (name, b, q, key, g, float(rf), err, bound)
                assert abs(g - r64_) <= 1e-6 * sz, (name, b, q, key, g, r64_, sz)
    print(f"{name}: largest err / bound " + ", ".join(f"{key} {v:.3g}" for key, v in worst.items()))


@pytest.mark.parametrize("name", CASES)
def test_every_pixel_and_width_against_the_float64_reference(name):
    c = case(name)
    N, wave, out = c["N"], np.asarray(c["o"]["wave"]), c["out"]
    worst = dict.fromkeys(KEYS, 0.0)
    for b in range(3):
        W64 = LS.cinv(c["C64"][b], np.float64)
        alpha64 = W64 @ c["resid"][b]
        for q, (mu, sg) in enumerate(c["cand"]):
            got = [out[key][b, q] for key in KEYS]
            if LS.patch(wave, mu, sg)[1] == 0:
                continue
            ref = LS.three(W64, alpha64, wave, mu, sg)
            size = LS.sizes(W64, alpha64, wave, mu, sg)
            for key, g, rf, sz in zip(KEYS, got, ref, size):
                worst[key] = max(worst[key], abs(g - rf) / sz)
                assert abs(g - rf) <= 1e-6 * sz, (name, b, q, key, g, rf, sz)
            assert got[2] > 0, (name, b, q, got)
    print(f"{name}: largest |got - float64 reference| / size " + ", ".join(f"{key} {v:.3g}" for key, v in worst.items()))
    # no pixel in reach: exactly zero
    for key in KEYS:
        assert (out[key][:, -1] == 0.0).all() and not np.signbit(out[key][:, -1]).any(), key


def test_same_bits_repeated_chunked_on_a_sub_batch_and_for_any_candidate_list():
    c = case("N180-full")
    do, md, rows, cand, out = c["do"], c["md"], c["rows"], c["cand"], c["out"]
    for other in (do.local_scan(md, rows, cand), do.local_scan(md, rows, cand, max_chunk=1)):
        for key in KEYS + ("lnl", "info"):
            np.testing.assert_array_equal(other[key], out[key], err_msg=key)
    sub = do.local_scan(md, rows[1:], cand)
    for key in KEYS + ("lnl", "info"):
        np.testing.assert_array_equal(sub[key], out[key][1:], err_msg=key)
    pick = np.random.default_rng(4).permutation(len(cand))[:97]
    some = do.local_scan(md, rows, cand[pick])
    for key in KEYS:
        np.testing.assert_array_equal(some[key], out[key][:, pick], err_msg=key)
    one = do.local_scan(md, rows[2:], cand[pick[:1]])
    for key in KEYS:
        np.testing.assert_array_equal(one[key], out[key][2:, pick[:1]], err_msg=key)


def test_the_workspace_has_the_documented_layout_and_no_term_quadratic_in_n_of_its_own():
    c = case("N180-full")
    do, md = c["do"], c["md"]
    q = do.local_scan_workspace_bytes
    assert do.npad == 192 and -(-do.n // 64) == 3
    assert q(md, 0, 5) == 0 and q(md, 3, 0) == 0 and q(md, 65536, 5) == 0 and q(md, 3, 65536) == 0
    assert (np.diff([q(md, B, 100) for B in (1, 2, 3, 64)]) > 0).all()
    assert (np.diff([q(md, 3, n) for n in (1, 100, 1000, 65535)]) > 0).all()
    # behind the head of the pointwise call (less its copy of the diagonal): two ints per candidate, then per walker and block
    # the 2 reach + 1 tiles of the band, reach = min(blocks - 1, 4)
    align = lambda x: -(-x // 256) * 256  # noqa: E731
    for name, nbr, reach in (("N180-full", 3, 2), ("N330-full", 6, 4)):
        k = case(name)
        for B in (1, 3, 64):
            own = k["do"].local_scan_workspace_bytes(k["md"], B, 100) - k["do"].pointwise_workspace_bytes(k["md"], B, 1)
            assert own == align(2 * 4 * 100) + 8 * B * nbr * (2 * reach + 1) * 4096 - align(8 * B * k["do"].npad), (name, B, own)
    # linear in n beyond the head: at a fixed reach the part of its own doubles with the blocks
    do12 = device_order(oracle_order(synth.make_order(N=768, m=4, seed=5)))
    md12 = do12.model_desc(True, True, True, False, 0, 2)
    own12 = do12.local_scan_workspace_bytes(md12, 2, 100) - do12.pointwise_workspace_bytes(md12, 2, 1) + align(8 * 2 * do12.npad)
    k = case("N330-full")
    own6 = k["do"].local_scan_workspace_bytes(k["md"], 2, 100) - k["do"].pointwise_workspace_bytes(k["md"], 2, 1) + align(8 * 2 * 384)
    assert do12.npad == 768 and own12 - align(800) == 2 * (own6 - align(800))


def test_refusals_that_need_a_context_name_the_call():
    import torch

    c = case("N180-none")
    do, md, rows, oo = c["do"], c["md"], c["rows"], c["oo"]
    cand = c["cand"][:7]
    need = do.local_scan_workspace_bytes(md, 3, 7)
    with torch.cuda.device(do.dev):
        Pd, Cd = D.to_dev(rows, do.dev), D.to_dev(cand, do.dev)
        out = torch.full((3, 7, 3), 77.0, dtype=torch.float64, device=do.dev)
        ws = do._reserve(need)
        args = (do.ctx, ctypes.byref(md), 3, D.ptr(Pd), D.ptr(Cd), 7, D.ptr(out), None, None, D.ptr(ws))
        rc = do.lib.sf_local_scan_batch(*args, need - 1, D.stream_ptr(do.dev))
        said = do.lib.sf_last_error().decode()
        assert rc == -2 and said.startswith("sf_local_scan_batch:") and "workspace too small" in said, (rc, said)
        torch.cuda.synchronize()
        assert (out == 77.0).all()
    perm = np.random.default_rng(12).permutation(180)
    shuffled = D.DeviceOrder(oo.wave[perm], oo.flux[perm], oo.sigma[perm], oo.min_dv_wave, oo.bulk_fluxes, oo.grid_points,
                             oo.variances, oo.lengthscales, oo.v11, oo.w_hat)
    assert shuffled.local_scan_workspace_bytes(md, 3, 7) == 0
    with pytest.raises(_lib.StarfishAMDError, match=r"sf_local_scan_batch: .*not monotonic"):
        shuffled.local_scan(md, rows, cand)


def test_a_patch_beyond_the_device_limit_is_nan_on_the_device_and_a_value_error_in_the_model():
    c = case("N330-full")
    do, md, rows, wave = c["do"], c["md"], c["rows"], np.asarray(c["o"]["wave"])
    wide = (float(wave[165]), 70.0)  # 4 sigma = 280 km/s on either side at 2 km/s pixels: 281 pixels
    lo, hi = D.local_scan_patches(wave, [wide, (float(wave[165]), 63.0)])
    assert hi[0] - lo[0] + 1 > D.LOCAL_SCAN_MAX_PATCH >= hi[1] - lo[1] + 1 > 250
    pick = np.array([5, 400, 3 * 330 + 1])
    cand = np.vstack([c["cand"][pick[:2]], [wide], c["cand"][pick[2:]], [(float(wave[165]), 63.0)]])
    out = do.local_scan(md, rows, cand)
    assert (out["info"] == 0).all()
    for key in KEYS:
        assert np.isnan(out[key][:, 2]).all(), key
        np.testing.assert_array_equal(out[key][:, [0, 1, 3]], c["out"][key][:, pick], err_msg=key)
    # the widest patch the device takes (five blocks): against the float64 reference
    for b in range(3):
        W64 = LS.cinv(c["C64"][b], np.float64)
        alpha64 = W64 @ c["resid"][b]
        ref, size = LS.three(W64, alpha64, wave, *cand[4]), LS.sizes(W64, alpha64, wave, *cand[4])
        for key, rf, sz in zip(KEYS, ref, size):
            assert abs(out[key][b, 4] - rf) <= 1e-6 * sz, (b, key, out[key][b, 4], rf, sz)
    model = synth.build_model(c["o"])
    with pytest.raises(ValueError, match=r"mu=.*sigma=70\.0 .*at most 256 pixels"):
        model.local_kernel_scan(mus=[wave[10], wave[165]], sigmas=(15.0, 70.0))
    with pytest.raises(ValueError, match="at most 256 pixels"):
        model.propose_local_kernels(sigmas=(70.0,))


def test_failed_walkers_get_nan_rows_and_leave_the_others_alone():
    """The mixed batch of tests/test_gpu_cov_fisher.py: data without pixel noise and log_scale 18 (not positive definite), T = 1e5
    (outside the grid)."""
    N = 256
    o = dict(synth.make_order(N=N, m=4, seed=5))
    o["sigma"] = np.zeros(N)
    model = synth.build_model(o)
    P = synth.walker_ball(o, B=3, seed=21)
    not_pd, off_grid = P[1].copy(), P[2].copy()
    not_pd[2] = 18.0
    off_grid[synth.LABELS.index("T")] = 1e5
    mixed = np.stack([P[0], not_pd, P[1], off_grid, P[2]])
    mus = o["wave"][::9]
    good, info0 = model.local_kernel_scan_batch(P, mus=mus, sigmas=SIGMAS, return_info=True)
    assert (info0 == 0).all() and all(np.isfinite(v).all() for v in good.values())
    got, info = model.local_kernel_scan_batch(mixed, mus=mus, sigmas=SIGMAS, return_info=True)
    _, info_ll = model.log_likelihood_batch(mixed, return_info=True)
    np.testing.assert_array_equal(info, info_ll)
    assert info[1] > 0 and info[3] == -1 and (info[[0, 2, 4]] == 0).all(), info
    for key, v in got.items():
        assert v.shape == (5, 3, len(mus)) and np.isnan(v[[1, 3]]).all(), key
        np.testing.assert_array_equal(v[[0, 2, 4]], good[key], err_msg=key)
    model.set_param_vector(not_pd)
    with pytest.raises(np.linalg.LinAlgError, match="leading minor"):
        model.local_kernel_scan(mus=mus)
    model.set_param_vector(off_grid)
    with pytest.raises(ValueError):
        model.propose_local_kernels()


def test_the_model_methods_hand_the_device_numbers_on_and_leave_the_model_alone():
    c = case("N180-full")
    model = synth.build_model(c["o"])
    l0 = model.log_likelihood()
    before = (len(model.residuals), model._lnprob, model._log_scale, model._glob_snapshot, model._loc_snapshot)
    wave = np.asarray(model.data.wave)
    far = wave[0] - 400 * (wave[1] - wave[0])
    mus = np.concatenate([wave[::5], [far]])
    res = model.local_kernel_scan_batch(c["P"], mus=mus, sigmas=SIGMAS)
    dev, md, rows = model._pack(c["P"], update_caches=False)
    raw = dev.local_scan(md, rows, np.array([(m, s) for s in SIGMAS for m in mus]))
    assert set(res) == {"score", "information", "z", "amp", "quad", "trace"}
    for key, dkey in (("quad", "quad"), ("trace", "trace"), ("information", "fisher")):
        np.testing.assert_array_equal(res[key], raw[dkey].reshape(3, 3, len(mus)), err_msg=key)
    np.testing.assert_array_equal(res["score"], 0.5 * (res["quad"] - res["trace"]))
    quad, trace, fisher = (res[key][..., :-1] for key in ("quad", "trace", "information"))
    np.testing.assert_array_equal(res["z"][..., :-1], 0.5 * (quad - trace) / np.sqrt(fisher))
    np.testing.assert_array_equal(res["amp"][..., :-1], res["score"][..., :-1] / fisher)
    assert (res["information"][..., -1] == 0).all() and np.isnan(res["z"][..., -1]).all() and np.isnan(res["amp"][..., -1]).all()
    assert (res["score"][..., -1] == 0).all()
    # the scalar form: the current parameters, every pixel by default, wl_range cuts the centres
    own = model.local_kernel_scan(sigmas=SIGMAS)
    dev, md, rows = model._pack(update_caches=False)
    raw = dev.local_scan(md, rows, np.array([(m, s) for s in SIGMAS for m in wave]))
    np.testing.assert_array_equal(own["information"], raw["fisher"][0].reshape(3, len(wave)))
    cut = model.local_kernel_scan(sigmas=SIGMAS, wl_range=(wave[20], wave[40]))
    for key in own:
        np.testing.assert_array_equal(cut[key], own[key][:, 20:41], err_msg=key)
    assert (len(model.residuals), model._lnprob, model._log_scale, model._glob_snapshot, model._loc_snapshot) == before
    assert model.log_likelihood() == l0


@pytest.mark.parametrize("N", [180, 330])
def test_a_line_in_the_data_is_proposed_once_and_nothing_on_the_untouched_order(N):
    o = dict(synth.make_order(N=N, m=4, seed=5))
    assert synth.build_model(o).propose_local_kernels(sigmas=SIGMAS) == []
    w = np.asarray(o["wave"])
    pix = 2 * N // 3 + 3
    o["flux"] = o["flux"] + 0.05 * np.exp(-0.5 * (O.C_KMS * (w - w[pix]) / w[pix] / 12.0) ** 2)
    model = synth.build_model(o)
    l0 = model.log_likelihood()
    before = (len(model.residuals), model._lnprob, model._log_scale, model._glob_snapshot, model._loc_snapshot,
              tuple(model.get_param_vector()), tuple(model.labels))
    scan = model.local_kernel_scan(sigmas=SIGMAS)
    print(f"N={N}: largest z per width {np.nanmax(scan['z'], axis=1)}, at pixels {np.nanargmax(scan['z'], axis=1)}")
    got = model.propose_local_kernels(sigmas=SIGMAS)
    print(f"N={N}: proposed {got}")
    assert len(got) == 1 and set(got[0]) == {"mu", "log_amp", "log_sigma"}
    assert abs(int(np.argmin(np.abs(w - got[0]["mu"]))) - pix) <= 1
    assert got[0]["log_sigma"] == np.log(15.0) and 0.5 * 0.05**2 <= np.exp(got[0]["log_amp"]) <= 2 * 0.05**2
    # over the walkers: the mean of z
    P = synth.walker_ball(o, B=3, seed=3)
    assert [k["mu"] for k in model.propose_local_kernels(sigmas=SIGMAS, P=P)] == [got[0]["mu"]]
    assert model.propose_local_kernels(sigmas=SIGMAS, max_kernels=0) == [] and model.propose_local_kernels(sigmas=SIGMAS, threshold=50.0) == []
    after = (len(model.residuals), model._lnprob, model._log_scale, model._glob_snapshot, model._loc_snapshot,
             tuple(model.get_param_vector()), tuple(model.labels))
    assert after == before and model.log_likelihood() == l0
    model["local_cov"] = [*model._local_kernels(), *got]
    l1 = model.log_likelihood()
    print(f"N={N}: lnL {l0!r} -> {l1!r} with the proposed kernel")
    assert l1 > l0
