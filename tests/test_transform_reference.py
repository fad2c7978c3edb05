"""CPU checks of the cases and tolerances behind tests/test_gpu_transform_chain.py: the order builders reach the FFT
lengths and kernel branches they claim, the Gray-kernel bound really bounds the fp64 formula (against mpmath), the
collocation norms are what the tolerances assume, and every GPU case could see a 1 % change of vsini, 1 km/s of vz or
1e-3 of a Chebyshev coefficient (> 100x its tolerance) -- so that none of them is a silent no-op."""
import mpmath
import numpy as np
import pytest

import transform_cases as TC
from oracle import sf_oracle as O
from starfish_amd import synth


def test_builders_reach_the_fft_lengths_and_branches():
    for nf in TC.HOT_NFS:
        o, oo = TC.case_order("nf", nf)
        assert len(oo.min_dv_wave) == nf
        assert len(o["wave"]) <= 4096 and np.all(np.diff(o["wave"]) > 0)
        br = TC.branch(nf)
        L = nf // 2
        assert br == dict(L=L, half_lds=nf <= 16384, half_odd=int(np.log2(L)) % 2 == 1, full_lds=nf <= 8192)
    # every combination of the hot path's LDS / global and odd / even stage count is reached
    seen = {(TC.branch(nf)["half_lds"], TC.branch(nf)["half_odd"]) for nf in TC.HOT_NFS}
    assert seen == {(True, True), (True, False), (False, True), (False, False)}
    assert TC.branch(16384) == dict(L=8192, half_lds=True, half_odd=True, full_lds=False)  # the largest LDS transform
    # spline bands with fewer 16-point blocks than the band's 9
    assert [nf for nf in TC.HOT_NFS if nf // 16 < 9] == [16, 32, 64, 128]
    for m in TC.MS:
        o, oo = TC.case_order("m", m)
        assert len(oo.min_dv_wave) == 2048 and oo.m == m
    for n in TC.RENORM_PIXELS:
        o, oo = TC.case_order("pixels", n)
        assert len(oo.wave) == n and len(oo.min_dv_wave) == {2: 16, 3: 32, 257: 512}[n]
    # the limits: synth.make_order reaches nf = 8 directly
    assert len(synth.make_order(N=6, m=4, seed=3, pad=0.04)["emu_wl"]) == 8


def test_far_doppler_shifts_leave_the_grid():
    for nf in (16384, 32768, 65536):
        _, oo = TC.case_order("nf", nf)
        for vz in (TC.VZ_FAR, -TC.VZ_FAR):
            assert TC.pixels_outside(oo, vz) > 0, (nf, vz)
        assert TC.pixels_outside(oo, 10.0) == TC.pixels_outside(oo, -10.0) == 0
        assert any(abs(p.get("vz", 0)) > 1000 for p in TC.case_walkers("nf", nf))
    for nf in (16, 32, 64, 1024):
        assert not any(abs(p.get("vz", 0)) > 1000 for p in TC.case_walkers("nf", nf))
    # the reference extrapolates those pixels with the end pieces: the Lebesgue factor grows there
    _, oo = TC.case_order("nf", 65536)
    p = [q for q in TC.walkers(8, far=True) if q["vz"] < -1000][0]
    r = TC.chain_reference(oo, p)
    assert r["lam"].max() > 1 and np.sum(r["lam"] > 1) == TC.pixels_outside(oo, p["vz"])


def test_walker_values():
    ws = TC.walkers(64, far=True)
    assert {round(p["vsini"] / (1 + 0.003 * (k // 4)), 9) for k, p in enumerate(ws)} == set(TC.VSINIS)
    vz = {p["vz"] for p in ws}
    assert any(v > 1000 for v in vz) and any(v < -1000 for v in vz) and 0.0 in vz
    assert len({repr(sorted(p.items())) for p in ws}) == len(ws)


def gray_exact(u):
    x = mpmath.mpf(float(u))
    return float(mpmath.besselj(1, x) / x - 3 * mpmath.cos(x) / (2 * x**2) + 3 * mpmath.sin(x) / (2 * x**3))


def test_rot_mult_bound_bounds_the_fp64_formula():
    mpmath.mp.dps = 50
    rng = np.random.default_rng(0)
    u = np.concatenate([np.logspace(-5, 1, 1500), 10 ** rng.uniform(-5, 1, 500)])
    err = np.abs(TC.gray_mult(u) - np.array([gray_exact(x) for x in u]))
    assert np.all(err <= TC.rot_mult_bound(u)), float(np.max(err / TC.rot_mult_bound(u)))
    # and it is not vacuous: within a factor 8 of the worst case where the cancellation dominates
    small = u < 1e-2
    assert np.max(err[small] / TC.rot_mult_bound(u[small])) > 1 / 8


def grids():
    rng = np.random.default_rng(5)
    for n in (6, 7, 20, 64, 200):
        step = np.full(n - 1, 2.0 / synth.C_KMS)
        yield 5000.0 * np.exp(np.concatenate([[0.0], np.cumsum(step)]))
        yield 5000.0 * np.exp(np.concatenate([[0.0], np.cumsum(step * (1 + 0.3 * rng.uniform(-1, 1, n - 1)))]))


def test_ainv_norm_is_the_dense_inverse_norm():
    for x in grids():
        Ainv = np.linalg.inv(TC.collocation_dense(x))
        n = len(x)
        sign = (-1.0) ** np.add.outer(np.arange(n), np.arange(n))
        assert np.all(Ainv * sign >= -1e-12 * np.abs(Ainv).max())  # checkerboard: A is totally positive
        want = np.abs(Ainv).sum(axis=1).max()
        assert abs(TC.ainv_norm(x) - want) <= 1e-12 * want
    # the log-uniform grids of the model: ||A^-1|| is set by the end rows, not by the interior's ~7.5
    for nf in (64, 2048, 65536):
        assert 6 < TC.ainv_norm(TC.case_order("nf", nf)[1].min_dv_wave) < 30


def test_amp_of_bins_is_the_worst_phase():
    x = TC.case_order("nf", 128)[1].min_dv_wave
    n = len(x)
    Ainv = np.linalg.inv(TC.collocation_dense(x))
    amp = TC.amp_of_bins(x)
    j = np.arange(n)
    for k in (1, 2, 5, 17, 40, 64):
        worst = max(np.abs(Ainv @ np.cos(2 * np.pi * k * j / n + phi)).max() for phi in np.linspace(0, np.pi, 721))
        assert worst <= amp[k - 1] * (1 + 1e-12) and amp[k - 1] <= worst * (1 + 1e-4), (k, worst, amp[k - 1])
    assert np.all(amp <= TC.ainv_norm(x) * (1 + 1e-12))
    assert amp[0] < 1.1  # a smooth error passes the fit almost unchanged


def test_resample_tolerance_holds_for_an_independent_solve():
    """The dense collocation solve (a different algorithm from FITPACK's) stays well inside resample_tol."""
    for x in grids():
        rng = np.random.default_rng(len(x))
        y = 1 + 0.05 * rng.standard_normal(len(x))
        h0, h1 = x[1] - x[0], x[-1] - x[-2]
        xq = np.concatenate([x, [x[0] - 2 * h0, x[-1] + 2 * h1], x[:-1] + 0.5 * np.diff(x)])
        c, t = O.quintic_collocation_fit(x, y)
        got = O.quintic_collocation_eval(t, c, xq)
        want = O.quintic_resample(x, y, xq)
        assert np.all(np.abs(got - want) <= TC.resample_tol(x, y, xq) / 8)


@pytest.mark.parametrize("label,kind,key,plist", TC.sensitivity_cases(), ids=[c[0] for c in TC.sensitivity_cases()])
def test_every_case_sees_a_small_parameter_change(label, kind, key, plist):
    _, oo = TC.case_order(kind, key)
    for p in plist:
        r = TC.chain_reference(oo, p)
        assert np.all(r["tol_flux"] > 0) and np.all(r["tol_X"] > 0)
        s = TC.sensitivity(oo, p, r["tol_flux"])
        assert s > 100, (label, p, s)


def test_free_broadening_cases_see_a_one_percent_vsini_change():
    for nf in (4, 8, 16, 16384, 32768, 65536):
        w = 5000.0 * np.exp(np.arange(nf) * TC.DV / synth.C_KMS)
        f = 1 + 0.1 * np.sin(w / 7)[None, :] + 0.05 * np.random.default_rng(nf).standard_normal((3, nf))
        for vsini in (0.5, 30.0, 300.0):
            want, tol = TC.broaden_reference(w, f, "rot", vsini)
            moved = O.rot_broaden(w, f, vsini * 1.01)
            assert np.max(np.abs(moved - want) / tol) > 100, (nf, vsini)
        want, tol = TC.broaden_reference(w, f, "inst", TC.kill_fwhm(nf, O.min_velocity_step(w)))
        assert np.ptp(want, axis=1).max() < 0.2 * np.ptp(f, axis=1).min()  # (the noise is gone)
