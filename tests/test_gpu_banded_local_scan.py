"""sf_local_scan_banded_batch through DeviceOrder.local_scan(solver="banded" | "auto") and the SpectrumModel methods: the score
scan of tests/test_gpu_local_scan.py from the band + Woodbury solver, W = C^-1 = Sigma - Vs Vs^T with Sigma = Bd^-1 from the
selected inversion at the LDS window's widest half-width wmax (144 for m = 4, 128 for m = 17) and Vs = Bd^-1 Y^T L_S^-T.

Cases: the six of the dense test (N = 180, 330 x full / global / none, m = 4, three walkers, the same candidates: patches of at most
121 pixels over one, two and three 64-blocks, clipped at both ends, one with no pixel in reach) and "N180-m17-full"
(synth.make_order(N=180, m=17, seed=5)), where the limit is 129 pixels.

The bound is the dense test's, with two changes.  There is no device factor of C: L is the longdouble Cholesky factor of the
oracle's matrix rounded to float64 and X its inverse (as tests/test_gpu_banded_cov_gradient.py takes them).  And |dW| gains
gamma_{m+1} (|Sigma| + |Vs||Vs|^T) on the patch for the subtraction Sigma_ij - sum_c Vs_ci Vs_cj (m products, m - 1 additions, one
subtraction; tests/test_gpu_banded_diagnostics.py adds the same term for the diagonal), Sigma and Vs from the longdouble
reference.  Against the dense call: |banded - dense| <= the sum of the two calls' own bounds.

Largest err / bound seen (quad, trace, fisher), banded: see DESIGN.md, "Score scan on the band solver"."""
import ctypes

import numpy as np
import pytest

from oracle import sf_oracle as O
from starfish_amd import _device as D
from starfish_amd import _lib, synth

import banded_derivatives as BD
import banded_diagnostics_reference as BR
import local_scan_reference as LS
import test_gpu_local_scan as DENSE
from gpu_helpers import device_order, oracle_order, pack_rows
from test_gpu_local_scan import SIGMAS, candidates
from test_gpu_model import close_lnl

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
KEYS = ("quad", "trace", "fisher")
M17 = "N180-m17-full"
CASES = DENSE.CASES + [M17]
LIMIT = {4: 145, 17: 129}  # sf_band_max_halfwidth(1 + m) + 1


def gamma(k):
    return k * U / (1 - k * U)


_CASES = {}


def case(name):
    """The dense test's case (its order, rows, candidates and dense results) with the banded results beside them; the m = 17
    case is built the same way.  Made once, never written."""
    if name not in _CASES:
        if name == M17:
            o = synth.make_order(N=180, m=17, seed=5)
            oo = oracle_order(o)
            do = device_order(oo)
            P = synth.walker_ball(o, B=3, seed=3)
            plist = [DENSE.oracle_params(name, p) for p in P]
            md, rows = pack_rows(do, plist)
            cand, subset = candidates(np.asarray(o["wave"]))
            c = dict(N=180, o=o, oo=oo, do=do, P=P, plist=plist, md=md, rows=rows, cand=cand, subset=subset)
            c["out"] = do.local_scan(md, rows, cand)
            c["resid"] = do.apply(md, rows, "Cinv", want_flux=True)["flux"] - oo.flux[None, :]
            c["C64"] = [O.forward_model(oo, p)[1] + O.JITTER * np.eye(180) for p in plist]
        else:
            c = dict(DENSE.case(name))
        c["m"] = int(c["do"].m)
        c["banded"] = c["do"].local_scan(c["md"], c["rows"], c["cand"], solver="banded")
        _CASES[name] = c
    return _CASES[name]


def bounds(c, b):
    """Per candidate of the subset of walker b: the longdouble reference, the float64 reference, the sizes and the bound of the
    dense call (own = 0) and of the banded call (own = the subtraction's term), from the reference alone.  Made once."""
    key = ("bounds", b)
    if key in c:
        return c[key]
    N, npad, m, wave = c["N"], c["do"].npad, c["m"], np.asarray(c["o"]["wave"])
    C64, r64 = c["C64"][b], c["resid"][b]
    L = LS.cholesky_longdouble(C64.astype(LD))
    X = LS.inverse_longdouble(L)
    W = X.T @ X
    alpha = W @ r64.astype(LD)
    W64 = LS.cinv(C64, np.float64)
    alpha64 = W64 @ r64
    aL, aX = np.abs(L).astype(np.float64), np.abs(X).astype(np.float64)  # (the reference factor rounded to float64)
    aW, aal = np.abs(W).astype(np.float64), np.abs(alpha).astype(np.float64)
    dC = 1e-13 * np.abs(C64) + gamma(npad + 1) * (aL @ aL.T)
    E = aX.T @ (aX @ (aL @ aX))
    dW_dense = aW @ dC @ aW + gamma(2 * npad) * (E + E.T) + gamma(npad + 1) * (aX.T @ aX)
    # Sigma = Bd^-1 and Vs of the oracle's pieces, in longdouble
    q = BD.pieces(c["oo"], c["plist"][b])
    XB = BR.inverse_lower(BR.cholesky(q["Bd"].astype(LD)))
    Sigma = XB.T @ XB
    TY = Sigma @ q["Y"].T.astype(LD)
    S = np.eye(q["Y"].shape[0], dtype=LD) + q["Y"].astype(LD) @ TY
    Vs = TY @ BR.inverse_lower(BR.cholesky(S)).T
    assert np.abs(Sigma - Vs @ Vs.T - W).max() <= 1e-10 * np.abs(W).max()  # (the identity the kernel evaluates)
    aVs = np.abs(Vs).astype(np.float64)
    dW_banded = dW_dense + gamma(m + 1) * (np.abs(Sigma).astype(np.float64) + aVs @ aVs.T)
    solve = (1e-13 + N * gamma(3 * N + 1)) * (np.abs(C64).sum(axis=1).max() * aal.max() + np.abs(r64).max())
    d_alpha = aW @ (dC @ aal) + aW.sum(axis=1) * solve
    rows = {}
    for qi in c["subset"]:
        mu, sg = c["cand"][qi]
        lo, hi, k = LS.patch_kernel(wave, mu, sg)
        if hi == lo:
            rows[qi] = None
            continue
        ref = LS.three(W, alpha, wave, mu, sg)
        ref64 = LS.three(W64, alpha64, wave, mu, sg)
        size = LS.sizes(W, alpha, wave, mu, sg)
        nblk = (hi - 1) // 64 - lo // 64 + 1
        Kq = 17 * (nblk * (nblk + 1) // 2) + 9
        Kf = 128 * nblk + Kq
        P = slice(lo, hi)
        rel = (1e-13 + 2 * U + gamma(Kq), 1e-13 + U + gamma(Kq), 2e-13 + 9 * U + gamma(Kf))
        both = []
        for dW in (dW_dense, dW_banded):
            first = (2 * d_alpha[P] @ k @ aal[P], np.sum(dW[P, P] * k),
                     0.5 * np.sum((dW[P, P] @ k @ aW[P, P] + aW[P, P] @ k @ dW[P, P]) * k))
            both.append([f1 + rl * sz for f1, rl, sz in zip(first, rel, size)])
        rows[qi] = dict(ref=[float(v) for v in ref], ref64=ref64, size=size, dense=both[0], banded=both[1])
    c[key] = dict(rows=rows, W64=W64, alpha64=alpha64)
    return c[key]


def test_the_candidates_lie_within_the_banded_limit_and_the_limit_is_the_windows():
    for name in CASES:
        c = case(name)
        do, md = c["do"], c["md"]
        lo, hi = D.local_scan_patches(c["o"]["wave"], c["cand"])
        assert (hi - lo + 1).max() <= 121 <= 145
        limit = do.local_scan_banded_max_patch(md)
        assert limit == LIMIT[c["m"]] == do.banded_window_halfwidth() + 1, (name, limit)
        assert (hi - lo + 1).max() <= limit
        assert (do.halfwidth_bound(md, c["rows"]) <= limit - 1).all()  # (no walker is refused: no case passes by falling back)


@pytest.mark.parametrize("name", CASES)
def test_lnl_info_and_shapes(name):
    c = case(name)
    out, dense = c["banded"], c["out"]
    assert (out["info"] == 0).all() and (dense["info"] == 0).all()
    np.testing.assert_array_equal(out["info"], dense["info"])
    for b in range(3):
        assert close_lnl(out["lnl"][b], dense["lnl"][b]), (name, b, out["lnl"][b], dense["lnl"][b])
    for key in KEYS:
        assert out[key].shape == (3, len(c["cand"])) and np.isfinite(out[key]).all(), key


@pytest.mark.parametrize("name", CASES)
def test_the_subset_within_its_bound_of_the_longdouble_reference_and_of_the_dense_call(name):
    c = case(name)
    worst = dict.fromkeys(KEYS, 0.0)
    worst_dense = dict.fromkeys(KEYS, 0.0)
    worst_pair = dict.fromkeys(KEYS, 0.0)
    for b in range(3):
        for q, row in bounds(c, b)["rows"].items():
            got = [c["banded"][key][b, q] for key in KEYS]
            den = [c["out"][key][b, q] for key in KEYS]
            if row is None:
                assert got == [0.0, 0.0, 0.0], (name, b, q, got)
                continue
            for i, key in enumerate(KEYS):
                err, err_d = abs(got[i] - row["ref"][i]), abs(den[i] - row["ref"][i])
                worst[key] = max(worst[key], err / row["banded"][i])
                worst_dense[key] = max(worst_dense[key], err_d / row["dense"][i])
                worst_pair[key] = max(worst_pair[key], abs(got[i] - den[i]) / (row["banded"][i] + row["dense"][i]))
    print(f"{name}: largest err / bound, banded " + ", ".join(f"{key} {v:.3g}" for key, v in worst.items()) + "; dense "
          + ", ".join(f"{key} {v:.3g}" for key, v in worst_dense.items()) + "; |banded - dense| / (sum of the two bounds) "
          + ", ".join(f"{key} {v:.3g}" for key, v in worst_pair.items()))
    for b in range(3):
        for q, row in bounds(c, b)["rows"].items():
            if row is None:
                continue
            for i, key in enumerate(KEYS):
                got, den = c["banded"][key][b, q], c["out"][key][b, q]
                assert abs(got - row["ref"][i]) <= row["banded"][i], (name, b, q, key, got, row["ref"][i], row["banded"][i])
                assert abs(got - row["ref64"][i]) <= 1e-6 * row["size"][i], (name, b, q, key, got, row["ref64"][i])
                assert abs(got - den) <= row["banded"][i] + row["dense"][i], (name, b, q, key, got, den)


@pytest.mark.parametrize("name", CASES)
def test_every_pixel_and_width_against_the_float64_reference(name):
    c = case(name)
    wave, out = np.asarray(c["o"]["wave"]), c["banded"]
    worst = dict.fromkeys(KEYS, 0.0)
    for b in range(3):
        ref_b = bounds(c, b)
        W64, alpha64 = ref_b["W64"], ref_b["alpha64"]
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
    for key in KEYS:  # no pixel in reach: exactly zero
        assert (out[key][:, -1] == 0.0).all() and not np.signbit(out[key][:, -1]).any(), key


@pytest.mark.parametrize("name", ["N180-full", M17])
def test_same_bits_repeated_chunked_on_a_sub_batch_and_for_any_candidate_list(name):
    c = case(name)
    do, md, rows, cand, out = c["do"], c["md"], c["rows"], c["cand"], c["banded"]
    kw = dict(solver="banded")
    for other in (do.local_scan(md, rows, cand, **kw), do.local_scan(md, rows, cand, max_chunk=1, **kw)):
        for key in KEYS + ("lnl", "info"):
            np.testing.assert_array_equal(other[key], out[key], err_msg=key)
    sub = do.local_scan(md, rows[1:], cand, **kw)
    for key in KEYS + ("lnl", "info"):
        np.testing.assert_array_equal(sub[key], out[key][1:], err_msg=key)
    pick = np.random.default_rng(4).permutation(len(cand))[:97]
    some = do.local_scan(md, rows, cand[pick], **kw)
    for key in KEYS:
        np.testing.assert_array_equal(some[key], out[key][:, pick], err_msg=key)
    one = do.local_scan(md, rows[2:], cand[pick[:1]], **kw)
    for key in KEYS:
        np.testing.assert_array_equal(one[key], out[key][2:, pick[:1]], err_msg=key)
    # "auto": every candidate and every walker fits, so it is the banded call; the dense call keeps its bits beside it
    auto = do.local_scan(md, rows, cand, solver="auto")
    again = do.local_scan(md, rows, cand)
    for key in KEYS + ("lnl", "info"):
        np.testing.assert_array_equal(auto[key], out[key], err_msg=key)
        np.testing.assert_array_equal(again[key], c["out"][key], err_msg=key)


def width_with(wave, pix, count):
    """(mu, sigma) around pixel ``pix`` whose patch has exactly ``count`` pixels (centres on and between pixels: odd and even)."""
    step = wave[pix + 1] - wave[pix]
    for off in (0.0, 0.5):
        mu = float(wave[pix] + off * step)
        sg = np.arange(4.0, 90.0, 0.05)
        lo, hi = D.local_scan_patches(wave, np.stack([np.full(sg.size, mu), sg], axis=1))
        hit = np.nonzero(hi - lo + 1 == count)[0]
        if hit.size:
            return mu, float(sg[hit[0]])
    raise AssertionError(f"no width with {count} pixels at pixel {pix}")


@pytest.mark.parametrize("name", ["N330-full", M17])
def test_the_limit(name):
    c = case(name)
    do, md, rows, wave = c["do"], c["md"], c["rows"], np.asarray(c["o"]["wave"])
    limit = do.local_scan_banded_max_patch(md)
    at, beyond = width_with(wave, c["N"] // 2, limit), width_with(wave, c["N"] // 2, limit + 1)
    lo, hi = D.local_scan_patches(wave, [at, beyond])
    assert hi[0] - lo[0] + 1 == limit and hi[1] - lo[1] + 1 == limit + 1 <= D.LOCAL_SCAN_MAX_PATCH
    pick = np.array([5, 2 * c["N"] + 7, 3 * c["N"] + 1])
    cand = np.vstack([c["cand"][pick[:2]], [beyond], c["cand"][pick[2:]], [at]])
    out = do.local_scan(md, rows, cand, solver="banded")
    assert (out["info"] == 0).all()
    for key in KEYS:
        assert np.isnan(out[key][:, 2]).all(), key
        np.testing.assert_array_equal(out[key][:, [0, 1, 3]], c["banded"][key][:, pick], err_msg=key)
    for b in range(3):  # the widest patch the band solver takes: against the float64 reference
        ref_b = bounds(c, b)
        ref, size = LS.three(ref_b["W64"], ref_b["alpha64"], wave, *at), LS.sizes(ref_b["W64"], ref_b["alpha64"], wave, *at)
        for key, rf, sz in zip(KEYS, ref, size):
            assert abs(out[key][b, 4] - rf) <= 1e-6 * sz, (b, key, out[key][b, 4], rf, sz)
    # "auto": one candidate beyond the limit sends the whole list to the dense call
    auto, dense = do.local_scan(md, rows, cand, solver="auto"), do.local_scan(md, rows, cand)
    for key in KEYS + ("lnl", "info"):
        np.testing.assert_array_equal(auto[key], dense[key], err_msg=key)
    assert np.isfinite(dense["fisher"][:, 2]).all()
    if name == M17:
        return
    model = synth.build_model(c["o"])
    mus, sigmas = [wave[10], beyond[0]], (15.0, beyond[1])
    with pytest.raises(ValueError, match=rf"mu=.*sigma={beyond[1]!r} km/s reaches {limit + 1} pixels.*at most {limit} pixels.*auto"):
        model.local_kernel_scan(mus=mus, sigmas=sigmas, solver="banded")
    with pytest.raises(ValueError, match=f"at most {limit} pixels"):
        model.propose_local_kernels(mus=mus, sigmas=sigmas, solver="banded")
    with pytest.raises(ValueError, match=f"at most {limit} pixels"):
        model.local_kernel_scan_batch(c["P"], mus=mus, sigmas=sigmas, solver="banded")
    got = model.local_kernel_scan(mus=mus, sigmas=sigmas, solver="auto")
    want = model.local_kernel_scan(mus=mus, sigmas=sigmas)
    for key in got:
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    with pytest.raises(ValueError, match="at most 256 pixels"):
        model.local_kernel_scan(mus=mus, sigmas=(70.0,), solver="auto")


def test_a_walker_wider_than_the_window_is_flagged_and_auto_sends_it_to_the_dense_call():
    c = case("N330-full")
    do, cand = c["do"], c["cand"][::11]
    plist = [dict(p) for p in c["plist"]]
    plist[1]["global_cov"] = (plist[1]["global_cov"][0], float(np.log(14.0)))
    md, rows = pack_rows(do, plist)
    hw = do.halfwidth_bound(md, rows)
    wmax = do.local_scan_banded_max_patch(md) - 1
    print("half-width bounds", hw)
    assert hw[1] > wmax and hw[0] <= wmax and hw[2] <= wmax
    out = do.local_scan(md, rows, cand, solver="banded")
    assert out["info"].tolist() == [0, D.INFO_BANDWIDTH, 0] and out["lnl"][1] == -np.inf
    for key in KEYS:
        assert np.isnan(out[key][1]).all(), key
        np.testing.assert_array_equal(out[key][[0, 2]], c["banded"][key][[0, 2]][:, ::11], err_msg=key)
    np.testing.assert_array_equal(out["lnl"][[0, 2]], c["banded"]["lnl"][[0, 2]])
    auto, dense = do.local_scan(md, rows, cand, solver="auto"), do.local_scan(md, rows, cand)
    assert (auto["info"] == 0).all()
    for key in KEYS + ("lnl",):
        np.testing.assert_array_equal(auto[key][1], dense[key][1], err_msg=key)
        np.testing.assert_array_equal(auto[key][[0, 2]], out[key][[0, 2]], err_msg=key)
    # the C-ABI itself: the fill's probe flags the walker the host bound would have kept away
    raw = do._local_scan_call("local_scan_banded_batch", md, rows, cand, None, do.local_scan_banded_workspace_bytes)
    assert raw["info"].tolist() == [0, D.INFO_BANDWIDTH, 0] and raw["lnl"][1] == -np.inf
    for key in KEYS:
        assert np.isnan(raw[key][1]).all(), key
        np.testing.assert_array_equal(raw[key][[0, 2]], out[key][[0, 2]], err_msg=key)


def test_failed_walkers_get_nan_rows_and_leave_the_others_alone():
    """The mixed batch of tests/test_gpu_local_scan.py: data without pixel noise and log_scale 18, T = 1e5 (outside the grid)."""
    N = 256
    o = dict(synth.make_order(N=N, m=4, seed=5))
    o["sigma"] = np.zeros(N)
    model = synth.build_model(o, solver="banded")
    P = synth.walker_ball(o, B=3, seed=21)
    not_pd, off_grid = P[1].copy(), P[2].copy()
    not_pd[2] = 18.0
    off_grid[synth.LABELS.index("T")] = 1e5
    mixed = np.stack([P[0], not_pd, P[1], off_grid, P[2]])
    mus = o["wave"][::9]
    good, info0 = model.local_kernel_scan_batch(P, mus=mus, sigmas=SIGMAS, return_info=True, solver="banded")
    assert (info0 == 0).all() and all(np.isfinite(v).all() for v in good.values())
    got, info = model.local_kernel_scan_batch(mixed, mus=mus, sigmas=SIGMAS, return_info=True, solver="banded")
    _, info_ll = model.log_likelihood_batch(mixed, return_info=True)
    print("info", info, "log_likelihood_batch on the band solver", info_ll)
    np.testing.assert_array_equal(info, info_ll)
    assert info[3] == -1 and (info[[0, 2, 4]] == 0).all(), info
    bad = np.nonzero(info != 0)[0]
    for key, v in got.items():
        assert v.shape == (5, 3, len(mus)) and np.isnan(v[bad]).all(), key
        np.testing.assert_array_equal(v[[0, 2, 4]], good[key], err_msg=key)


def test_the_workspace_has_the_documented_layout_and_is_linear_in_n():
    align = lambda x: -(-x // 256) * 256  # noqa: E731
    for name, nbr, reach in (("N180-full", 3, 2), ("N330-full", 6, 3), (M17, 3, 2)):
        c = case(name)
        do, md = c["do"], c["md"]
        q = do.local_scan_banded_workspace_bytes
        wmax = do.local_scan_banded_max_patch(md) - 1
        assert q(md, 0, 5) == 0 and q(md, 3, 0) == 0 and q(md, 65536, 5) == 0 and q(md, 3, 65536) == 0
        assert (np.diff([q(md, B, 100) for B in (1, 2, 3, 64)]) > 0).all()
        assert (np.diff([q(md, 3, n) for n in (1, 100, 1000, 65535)]) > 0).all()
        for B in (1, 3, 64):
            own = q(md, B, 100) - do.diagnose_banded_workspace_bytes(md, B, wmax, 1, True, False)
            assert own == align(2 * 4 * 100) + 8 * B * nbr * (2 * reach + 1) * 4096, (name, B, own)
    # linear in n: twice the blocks at the same reach, twice the tiles; the whole workspace less than twice as well
    do12 = device_order(oracle_order(synth.make_order(N=768, m=4, seed=5)))
    md12 = do12.model_desc(True, True, True, False, 0, 2)
    k = case("N330-full")
    own12 = do12.local_scan_banded_workspace_bytes(md12, 2, 100) - do12.diagnose_banded_workspace_bytes(md12, 2, 144, 1, True, False)
    own6 = k["do"].local_scan_banded_workspace_bytes(k["md"], 2, 100) - k["do"].diagnose_banded_workspace_bytes(k["md"], 2, 144, 1, True, False)
    assert do12.npad == 768 and own12 - align(800) == 2 * (own6 - align(800))


def test_every_refusal_names_the_call_and_enqueues_nothing():
    import torch

    c = case("N180-none")
    do, md, rows, oo = c["do"], c["md"], c["rows"], c["oo"]
    cand = c["cand"][:7]
    need = do.local_scan_banded_workspace_bytes(md, 3, 7)
    with torch.cuda.device(do.dev):
        Pd, Cd = D.to_dev(rows, do.dev), D.to_dev(cand, do.dev)
        out = torch.full((3, 7, 3), 77.0, dtype=torch.float64, device=do.dev)
        ws = do._reserve(need)

        def call(ctx=do.ctx, model=md, B=3, P=Pd, cd=Cd, ncand=7, o=out, work=ws, nbytes=need):
            rc = do.lib.sf_local_scan_banded_batch(ctx, ctypes.byref(model) if model is not None else None, B, D.ptr(P), D.ptr(cd), ncand,
                                                   D.ptr(o), None, None, D.ptr(work), nbytes, D.stream_ptr(do.dev))
            return rc, do.lib.sf_last_error().decode()

        refused = [(dict(B=0), -1, "B=0"), (dict(B=65536), -1, "B=65536"), (dict(ncand=0), -1, "ncand=0"),
                   (dict(ncand=65536), -1, "ncand=65536"), (dict(P=None), -1, "required"), (dict(cd=None), -1, "required"),
                   (dict(o=None), -1, "required"), (dict(work=None), -1, "required"), (dict(ctx=None), -1, "bad context"),
                   (dict(model=None), -1, "bad context"), (dict(nbytes=need - 1), -2, "workspace too small")]
        for kw, code, word in refused:
            rc, said = call(**kw)
            assert rc == code and said.startswith("sf_local_scan_banded_batch:") and word in said, (kw, rc, said)
        torch.cuda.synchronize()
        assert (out == 77.0).all()
        rc, said = call()
        torch.cuda.synchronize()
        assert rc == 0 and not (out == 77.0).any(), (rc, said)
    assert do.local_scan_banded_workspace_bytes(md, 3, 7) == need
    perm = np.random.default_rng(12).permutation(180)
    shuffled = D.DeviceOrder(oo.wave[perm], oo.flux[perm], oo.sigma[perm], oo.min_dv_wave, oo.bulk_fluxes, oo.grid_points,
                             oo.variances, oo.lengthscales, oo.v11, oo.w_hat)
    assert shuffled.local_scan_banded_workspace_bytes(md, 3, 7) == 0 and shuffled.local_scan_banded_max_patch(md) == 0
    with pytest.raises(_lib.StarfishAMDError, match=r"sf_local_scan_banded_batch: .*not monotonic"):
        shuffled._local_scan_call("local_scan_banded_batch", md, rows, cand, None, shuffled.local_scan_banded_workspace_bytes)
    with pytest.raises(ValueError, match="does not take this order"):
        shuffled.local_scan(md, rows, cand, solver="banded")


def test_the_model_methods_hand_the_device_numbers_on_and_leave_the_model_alone():
    c = case("N180-full")
    model = synth.build_model(c["o"], solver="auto")
    l0 = model.log_likelihood()
    before = (len(model.residuals), model._lnprob, model._log_scale, model._glob_snapshot, model._loc_snapshot)
    wave = np.asarray(model.data.wave)
    far = wave[0] - 400 * (wave[1] - wave[0])
    mus = np.concatenate([wave[::5], [far]])
    cand = np.array([(m, s) for s in SIGMAS for m in mus])
    dev, md, rows = model._pack(c["P"], update_caches=False)
    dense, banded = dev.local_scan(md, rows, cand), dev.local_scan(md, rows, cand, solver="banded")
    assert not np.array_equal(dense["quad"], banded["quad"])  # (to rounding, not bit for bit: the two can be told apart)
    for solver, raw in ((None, dense), ("dense", dense), ("auto", banded), ("banded", banded)):
        res, info = model.local_kernel_scan_batch(c["P"], mus=mus, sigmas=SIGMAS, return_info=True, solver=solver)
        assert set(res) == {"score", "information", "z", "amp", "quad", "trace"} and (info == 0).all()
        for key, dkey in (("quad", "quad"), ("trace", "trace"), ("information", "fisher")):
            np.testing.assert_array_equal(res[key], raw[dkey].reshape(3, 3, len(mus)), err_msg=f"{solver} {key}")
        assert (res["information"][..., -1] == 0).all() and np.isnan(res["z"][..., -1]).all()
    own = model.local_kernel_scan(sigmas=SIGMAS, solver="auto")
    dev, md, rows = model._pack(update_caches=False)
    raw = dev.local_scan(md, rows, np.array([(m, s) for s in SIGMAS for m in wave]), solver="banded")
    np.testing.assert_array_equal(own["information"], raw["fisher"][0].reshape(3, len(wave)))
    with pytest.raises(ValueError, match="solver must be"):
        model.local_kernel_scan(solver="band")
    assert (len(model.residuals), model._lnprob, model._log_scale, model._glob_snapshot, model._loc_snapshot) == before
    assert model.log_likelihood() == l0


@pytest.mark.parametrize("N", [180, 330])
def test_a_line_in_the_data_is_proposed_once_with_the_band_solver_as_without(N):
    o = dict(synth.make_order(N=N, m=4, seed=5))
    assert synth.build_model(o).propose_local_kernels(sigmas=SIGMAS, solver="auto") == []
    w = np.asarray(o["wave"])
    pix = 2 * N // 3 + 3
    o["flux"] = o["flux"] + 0.05 * np.exp(-0.5 * (O.C_KMS * (w - w[pix]) / w[pix] / 12.0) ** 2)
    model = synth.build_model(o)
    l0 = model.log_likelihood()
    dense = model.propose_local_kernels(sigmas=SIGMAS)
    got = model.propose_local_kernels(sigmas=SIGMAS, solver="auto")
    print(f"N={N}: proposed {got} (dense factor: {dense})")
    assert len(got) == 1 == len(dense) and got[0]["mu"] == dense[0]["mu"] and got[0]["log_sigma"] == dense[0]["log_sigma"] == np.log(15.0)
    assert abs(got[0]["log_amp"] - dense[0]["log_amp"]) <= 1e-9
    assert abs(int(np.argmin(np.abs(w - got[0]["mu"]))) - pix) <= 1
    assert model.log_likelihood() == l0
