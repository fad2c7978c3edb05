"""The score scan for new local kernels without a device: the new C-ABI names, what sf_local_scan_batch refuses before it looks
at a context, the numpy helper of the GPU test (tests/local_scan_reference.py) against routes that use none of its formulas, the
host copy of the device's patch search, and the peak picking of SpectrumModel.propose_local_kernels as a pure function."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import sf_oracle as O
from starfish_amd import _device as D
from starfish_amd import _lib, synth
from starfish_amd.models import SpectrumModel
from starfish_amd.models._diagnostics import pick_local_kernels

import local_scan_reference as LS
from gpu_helpers import oracle_order

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
NEW_NAMES = {"sf_local_scan_workspace_bytes": 4, "sf_local_scan_batch": 12, "sf_debug_local_scan_contract": 10}
EINVAL, FAKE = -1, 0x10000  # (a pointer that is not NULL; the calls below return before they read it)
LD = np.longdouble


def test_new_entry_points_are_declared_bound_and_exported():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "starfish_amd.h")).read()
    for name, nargs in NEW_NAMES.items():
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        declared = re.search(rf"^(?:size_t|int) {name}\s*\(([^;]*)\);", header, re.M)
        assert declared and declared.group(1).count(",") + 1 == nargs, name
    for name in ("local_kernel_scan", "local_kernel_scan_batch", "propose_local_kernels"):
        assert callable(getattr(SpectrumModel, name, None)), name
    for name in ("local_scan", "local_scan_workspace_bytes"):
        assert callable(getattr(D.DeviceOrder, name, None)), name
    limit = re.search(r"#define\s+SF_LOCAL_SCAN_MAX_PATCH\s+(\d+)", header)
    assert limit and int(limit.group(1)) == D.LOCAL_SCAN_MAX_PATCH >= 256


# ------------------------------------------------------------------------------------------ refusals
def model_desc(has_global=0, n_local=0):
    md = _lib.ModelDesc()
    md.has_global, md.n_local = has_global, n_local
    return md


GOOD = dict(B=3, params=FAKE, cand=FAKE, ncand=5, out=FAKE)
BAD = [(dict(B=0), "B=0"), (dict(B=-2), "B=-2"), (dict(B=65536), "B=65536"), (dict(ncand=0), "ncand=0"), (dict(ncand=-1), "ncand=-1"),
       (dict(ncand=65536), "ncand=65536"), (dict(params=None), "required"), (dict(cand=None), "required"), (dict(out=None), "required")]


def local_scan_rc(lib, **kw):
    a = dict(GOOD, **kw)
    return lib.sf_local_scan_batch(None, C.byref(model_desc()), a["B"], a["params"], a["cand"], a["ncand"], a["out"], None, None,
                                   FAKE, 1 << 40, None)


@pytest.mark.parametrize("kw,word", BAD)
def test_local_scan_refuses_before_it_looks_at_the_context(kw, word):
    lib = _lib.load()
    assert local_scan_rc(lib, **kw) == EINVAL, kw
    msg = lib.sf_last_error().decode()
    assert msg.startswith("sf_local_scan_batch:") and word in msg, (kw, msg)
    a = dict(GOOD, **kw)
    assert lib.sf_local_scan_workspace_bytes(None, C.byref(model_desc()), a["B"], a["ncand"]) == 0
    rc = lib.sf_debug_local_scan_contract(None, C.byref(model_desc()), a["B"], a["params"], a["cand"], a["ncand"], a["out"], FAKE,
                                          1 << 40, None)
    assert rc == EINVAL and lib.sf_last_error().decode().startswith("sf_debug_local_scan_contract:")


def test_with_good_counts_the_missing_context_is_what_is_refused_whatever_kernels_the_model_has():
    """No "nothing to differentiate" refusal: a model without any structured kernel gets as far as one with both (d_lnl and
    d_info may be NULL)."""
    lib = _lib.load()
    for kernels in ((0, 0), (1, 0), (1, 1), (0, 2)):
        rc = lib.sf_local_scan_batch(None, C.byref(model_desc(*kernels)), 3, FAKE, FAKE, 5, FAKE, None, None, FAKE, 1 << 40, None)
        assert rc == EINVAL and lib.sf_last_error().decode() == "bad context / model descriptor", kernels
        assert lib.sf_local_scan_workspace_bytes(None, C.byref(model_desc(*kernels)), 3, 5) == 0
    assert lib.sf_local_scan_workspace_bytes(None, None, 3, 5) == 0


# ------------------------------------------------------------------------------------------ the helper
def order_and_matrix(N, line=False):
    """The order of the GPU test (m = 4, seed 5), walker 0 of walker_ball(seed=3): wave, residual, C with jitter, parameters."""
    o = dict(synth.make_order(N=N, m=4, seed=5))
    if line:
        w = o["wave"]
        c = 2 * N // 3 + 3
        o["flux"] = o["flux"] + 0.05 * np.exp(-0.5 * (O.C_KMS * (w - w[c]) / w[c] / 12.0) ** 2)
    oo = oracle_order(o)
    p = synth.vector_to_oracle_params(synth.walker_ball(o, B=3, seed=3)[0])
    flux, cov, _ = O.forward_model(oo, p)
    return o["wave"], flux - oo.flux, cov + O.JITTER * np.eye(N), oo, p


@pytest.mark.parametrize("N", [180, 330])
def test_the_helper_is_the_derivative_of_the_likelihood_and_the_trace_formed_the_long_way(N):
    """U = 1/2 (quad - trace) against the central difference of lnL(C + A k) = -1/2 (logdet + r^T (C + A k)^-1 r), the Cholesky
    factor of the float64 matrix taken in longdouble, with steps h and h / 2 and one Richardson step.  The natural scale of A is
    1 / sqrt(fisher) (lnL changes by order 1 over it), so h = 1e-2 / sqrt(fisher): the Richardson remainder is of order (h
    sqrt(fisher))^4 = 1e-8 of the derivative's scale, the rounding of the difference 2^-64 |lnL| / h, below 1e-9 of it.  Agreement
    to 1e-6 (size_quad + size_trace).  fisher against 1/2 tr(W k W k) from the full N x N matrices."""
    wave, r, Cj, _, _ = order_and_matrix(N)
    W = LS.cinv(Cj)
    alpha = W @ r.astype(LD)
    CL = Cj.astype(LD)
    rl = r.astype(LD)

    def lnl(K, A):
        L = LS.cholesky_longdouble(CL + LD(A) * K)
        z = LS.inverse_longdouble(L) @ rl
        return -(2 * np.sum(np.log(np.diag(L))) + z @ z) / 2

    worst = 0.0
    for pix, sigma in ((5, 8.0), (N // 3 + 2, 15.0), (64, 30.0), (N - 2, 15.0), (2 * N // 3 + 3, 15.0)):
        mu = float(wave[pix] + 0.3 * (wave[1] - wave[0]))
        K = LS.kernel(wave, mu, sigma).astype(LD)
        lo, hi = LS.patch(wave, mu, sigma)
        mask = np.zeros((N, N), dtype=bool)
        mask[lo:hi, lo:hi] = True
        assert (K[~mask] == 0).all() and np.array_equal(K[lo:hi, lo:hi].astype(np.float64), LS.patch_kernel(wave, mu, sigma)[2])
        quad, trace, fisher = LS.three(W, alpha, wave, mu, sigma)
        sq, st, sf = LS.sizes(W, alpha, wave, mu, sigma)
        U = 0.5 * (quad - trace)
        h = 1e-2 / float(np.sqrt(fisher))
        d1 = (lnl(K, h) - lnl(K, -h)) / (2 * h)
        d2 = (lnl(K, h / 2) - lnl(K, -h / 2)) / h
        cd = (4 * d2 - d1) / 3
        ratio = abs(float(U - cd)) / (sq + st)
        long_way = 0.5 * np.trace(W @ K @ W @ K)
        print(f"N={N} pixel {pix} sigma {sigma}: U = {float(U):.12g}, central difference = {float(cd):.12g}, |difference| / size = "
              f"{ratio:.3g}; fisher = {float(fisher):.12g}, the long way {float(long_way):.12g}")
        worst = max(worst, ratio)
        assert ratio <= 1e-6
        assert abs(float(fisher - long_way)) <= 1e-12 * sf and 0 < fisher <= sf * (1 + 1e-12)
        assert abs(quad) <= sq * (1 + 1e-12) and abs(trace) <= st * (1 + 1e-12)
        # the float64 form
        W64 = LS.cinv(Cj, np.float64)
        got64 = LS.three(W64, W64 @ r, wave, mu, sigma)
        for a, b, s in zip(got64, (quad, trace, fisher), (sq, st, sf)):
            assert abs(float(a - b)) <= 1e-6 * s
    print(f"N={N}: worst |U - central difference| / size {worst:.3g}")


def test_the_score_finds_an_injected_line_and_stays_quiet_without_one():
    """The figures of the issue at N = 180: without a feature no z above 4 over every pixel and the three widths; with a Gaussian
    line of height 0.05 and width 12 km/s at pixel 2N/3 + 3 the largest z is above 4, within one pixel of the line and at sigma =
    15 km/s, with the Newton amplitude within a factor 2 of 0.05^2."""
    N = 180
    best = {}
    for line in (False, True):
        wave, r, Cj, _, _ = order_and_matrix(N, line)
        W = LS.cinv(Cj, np.float64)
        alpha = W @ r
        z = np.zeros((3, N))
        amp = np.zeros((3, N))
        for s, sigma in enumerate((8.0, 15.0, 30.0)):
            for j in range(N):
                quad, trace, fisher = LS.three(W, alpha, wave, wave[j], sigma)
                z[s, j] = 0.5 * (quad - trace) / np.sqrt(fisher)
                amp[s, j] = 0.5 * (quad - trace) / fisher
        s, j = np.unravel_index(np.argmax(z), z.shape)
        best[line] = (z[s, j], s, j, amp[s, j])
        print(f"line={line}: max z = {z[s, j]:.3f} at pixel {j}, width index {s}, amp = {amp[s, j]:.3e}")
        picked = pick_local_kernels(z, amp, wave, (8.0, 15.0, 30.0))
        if line:
            assert len(picked) == 1 and abs(np.searchsorted(wave, picked[0]["mu"]) - (2 * N // 3 + 3)) <= 1
            assert picked[0]["log_sigma"] == np.log(15.0) and 0.5 * 0.05**2 <= np.exp(picked[0]["log_amp"]) <= 2 * 0.05**2
        else:
            assert picked == []
    assert best[False][0] < 4.0 < best[True][0]
    assert best[True][1] == 1 and abs(best[True][2] - (2 * N // 3 + 3)) <= 1


# ------------------------------------------------------------------------------------------ the device's patch search on the host
def test_host_patches_are_the_pixels_within_four_sigma_with_the_margin_of_the_support_test():
    wave = np.asarray(synth.make_order(N=330, m=4, seed=5)["wave"])
    step = wave[1] - wave[0]
    cand = [(wave[0], 8.0), (wave[100] + 0.3 * step, 15.0), (wave[329], 30.0), (wave[0] - 20 * step, 15.0), (wave[0] - 500 * step, 15.0),
            (wave[329] + 500 * step, 8.0), (wave[150], 200.0), (wave[150], 1e-3), (wave[150] + 0.5 * step, 1e-3)]
    lo, hi = D.local_scan_patches(wave, cand)
    for q, (mu, sg) in enumerate(cand):
        want = np.nonzero(O.C_KMS / mu * np.abs(wave - mu) <= 4 * sg * (1 + 1e-9))[0]
        if want.size:
            assert (lo[q], hi[q]) == (want[0], want[-1]), q
            assert np.array_equal(want, np.arange(want[0], want[-1] + 1))
        else:
            assert hi[q] < lo[q], q
    assert hi[4] < lo[4] and hi[5] < lo[5] and hi[8] < lo[8] and (lo[7], hi[7]) == (150, 150)
    assert hi[6] - lo[6] + 1 > D.LOCAL_SCAN_MAX_PATCH  # 200 km/s at 2 km/s pixels: 800 pixels, clipped by the order to 330
    # the patch of the reference helper (no margin) lies inside
    for q, (mu, sg) in enumerate(cand[:4]):
        a, b = LS.patch(wave, mu, sg)
        assert lo[q] <= a and b - 1 <= hi[q]
    # a grid that is not sorted: the full search
    shuffled = wave[::-1].copy()
    lo2, hi2 = D.local_scan_patches(shuffled, cand[:3])
    assert np.array_equal(lo2, 329 - hi[:3]) and np.array_equal(hi2, 329 - lo[:3])


# ------------------------------------------------------------------------------------------ peak picking
MUS = 5000.0 + 0.03 * np.arange(40)  # about 1.8 km/s per step: sigma = 15 km/s reaches 4 * 15 * 5000 / c = 1.0 = 33 steps
SIG = (8.0, 15.0, 30.0)


def flat(value=0.0):
    return np.full((3, 40), value), np.full((3, 40), 1e-3)


def test_picking_keeps_what_is_above_the_threshold_with_the_best_width_sorted_by_mu():
    z, amp = flat()
    z[1, 5], amp[1, 5] = 6.0, 2e-3
    z[0, 5] = 5.0
    z[2, 30], amp[2, 30] = 4.5, 3e-3
    z[0, 20] = 4.0  # (not above the threshold)
    got = pick_local_kernels(z, amp, MUS, SIG, buffer=0.1)
    assert got == [dict(mu=MUS[5], log_amp=np.log(2e-3), log_sigma=np.log(15.0)), dict(mu=MUS[30], log_amp=np.log(3e-3), log_sigma=np.log(30.0))]
    assert pick_local_kernels(z, amp, MUS, SIG, threshold=3.9, buffer=0.1)[1]["mu"] == MUS[20]
    assert pick_local_kernels(z, amp, MUS, SIG, threshold=6.0) == []
    assert pick_local_kernels(*flat(), MUS, SIG) == []


def test_picking_drops_centres_within_the_buffer_of_a_kept_one():
    z, amp = flat()
    z[1, 10:15] = [5.0, 7.0, 9.0, 7.5, 5.5]  # one feature, five pixels above the threshold
    z[0, 36] = 4.2  # 24 steps = 0.72 from the peak: inside the reach of sigma = 15 km/s (1.0), outside that of 8 km/s (0.53)
    assert [k["mu"] for k in pick_local_kernels(z, amp, MUS, SIG)] == [MUS[12]]
    assert [k["mu"] for k in pick_local_kernels(z, amp, MUS, SIG, buffer=0.5)] == [MUS[12], MUS[36]]
    assert [k["mu"] for k in pick_local_kernels(z, amp, MUS, SIG, buffer=0.045)] == [MUS[10], MUS[12], MUS[14], MUS[36]]
    # the default buffer is the KEPT kernel's reach: a narrow kept kernel lets a wide neighbour outside its own reach stand
    z2, amp2 = flat()
    z2[0, 5], z2[2, 30] = 9.0, 5.0  # 25 steps = 0.75 apart: beyond 4 * 8 km/s (0.53), within 4 * 30 km/s (2.0)
    assert [k["mu"] for k in pick_local_kernels(z2, amp2, MUS, SIG)] == [MUS[5], MUS[30]]
    z2[0, 5], z2[2, 30] = 5.0, 9.0
    assert [k["mu"] for k in pick_local_kernels(z2, amp2, MUS, SIG)] == [MUS[30]]


def test_picking_breaks_ties_towards_the_first_width_and_the_smaller_mu_and_stops_at_max_kernels():
    z, amp = flat()
    z[:, 8] = 6.0  # the same z at every width: the first
    z[1, 30] = 6.0  # the same z at another centre: the smaller mu is walked first
    got = pick_local_kernels(z, amp, MUS, SIG, buffer=0.1)
    assert [(k["mu"], k["log_sigma"]) for k in got] == [(MUS[8], np.log(8.0)), (MUS[30], np.log(15.0))]
    assert [k["mu"] for k in pick_local_kernels(z, amp, MUS, SIG, buffer=0.1, max_kernels=1)] == [MUS[8]]
    z[1, 20] = 7.0
    assert [k["mu"] for k in pick_local_kernels(z, amp, MUS, SIG, buffer=0.1, max_kernels=2)] == [MUS[8], MUS[20]]
    assert pick_local_kernels(z, amp, MUS, SIG, max_kernels=0) == []
    assert len(pick_local_kernels(z, amp, MUS, SIG, buffer=0.1, max_kernels=None)) == 3


def test_picking_ignores_nan_and_candidates_without_a_positive_amplitude():
    z, amp = flat()
    z[:, 3], amp[:, 3] = np.nan, np.nan  # a centre with no pixel in reach at any width
    z[0, 12], amp[0, 12] = np.nan, np.nan
    z[1, 12], amp[1, 12] = 5.0, 1e-3  # NaN at one width only: the others count
    z[2, 25], amp[2, 25] = 8.0, np.nan
    z[2, 33], amp[2, 33] = 8.0, 0.0
    got = pick_local_kernels(z, amp, MUS, SIG, buffer=0.1)
    assert [(k["mu"], k["log_sigma"]) for k in got] == [(MUS[12], np.log(15.0))]
    with pytest.raises(ValueError, match="expected"):
        pick_local_kernels(z[:2], amp, MUS, SIG)
