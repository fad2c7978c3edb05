"""The transform chain of sf_transform_batch (emulator -> rotational broadening -> spline fit -> Doppler-shifted spline
evaluation -> Chebyshev / extinction -> scale) and the free transforms across the size-dependent branches of
sf_transform.hip: FFT lengths from 4 to 65536 (LDS and global scratch, odd and even radix-4 stage counts, the full-length
free-function transform beyond 8192), spline bands narrower than their 9 blocks, one to three column blocks of
k_spline_apply, walker chunks with odd tails, Doppler shifts past the ends of the grid, the renormalised scale at 2, 3
and 257 pixels, k_spline_solve's partial 64-lane waves.  Every comparison uses the per-element tolerance of
tests/transform_cases.py (derived from error bounds; tests/test_transform_reference.py checks the bounds and that each
case could see a 1 % change of vsini, 1 km/s of vz or 1e-3 of a Chebyshev coefficient).  Needs an MI355X: run with
-m gpu."""
import functools

import numpy as np
import pytest

import transform_cases as TC
from gpu_helpers import device_order, pack_rows
from oracle import sf_oracle as O
from starfish_amd import _device as D
from starfish_amd import _lib, synth
from starfish_amd import transforms as T

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def case_device(kind, key):
    o, oo = TC.case_order(kind, key)
    return device_order(oo)


_refs = {}


def reference(kind, key, oo, p):
    k = (kind, key, repr(sorted(p.items())))
    if k not in _refs:
        _refs[k] = TC.chain_reference(oo, p)
    return _refs[k]


def check_chain(kind, key, plist, out, where=""):
    _, oo = TC.case_order(kind, key)
    for b, p in enumerate(plist):
        r = reference(kind, key, oo, p)
        assert out["info"][b] == 0, (where, b, out["info"])
        ef = np.abs(out["flux"][b] - r["flux"]) / r["tol_flux"]
        assert ef.max() <= 1, (where, b, p, float(ef.max()), int(ef.argmax()))
        ex = np.abs(out["X"][b] - r["X"]) / r["tol_X"]
        assert ex.max() <= 1, (where, b, p, float(ex.max()), np.unravel_index(ex.argmax(), ex.shape))
        er = np.abs(out["resid"][b] - (r["flux"] - oo.flux)) / (r["tol_flux"] + 4 * TC.EPS * np.abs(oo.flux))
        assert er.max() <= 1, (where, b, float(er.max()))
        if "log_scale" in p:
            assert out["log_scale"][b] == p["log_scale"], (where, b)
        else:
            assert abs(out["log_scale"][b] - r["log_scale"]) <= r["tol_log_scale"], (where, b, out["log_scale"][b], r["log_scale"])


def run_chain(kind, key, plist):
    do = case_device(kind, key)
    md, rows = pack_rows(do, plist)
    return do, md, rows, do.transform(md, rows)


# ------------------------------------------------------------------------------------------------ hot path
@pytest.mark.parametrize("nf", TC.HOT_NFS)
def test_transform_across_fft_lengths(nf):
    """Four walkers (vsini 0.5, 2, 30, 300; vz 0 and +-10 or +-1500 km/s) at every FFT length of the hot path."""
    br = TC.branch(nf)
    assert br["L"] == nf // 2
    plist = TC.case_walkers("nf", nf)
    _, oo = TC.case_order("nf", nf)
    if nf >= 16384:
        far = [p for p in plist if abs(p["vz"]) > 1000]
        assert far and all(TC.pixels_outside(oo, p["vz"]) > 0 for p in far)
    *_, out = run_chain("nf", nf, plist)
    check_chain("nf", nf, plist, out, f"nf={nf} {br}")


@pytest.mark.parametrize("m", TC.MS)
def test_transform_across_emulator_rank(m):
    """m + 2 = 3 .. 34 rows: one, two and three column blocks of k_spline_apply (the second pass from 33 rows on)."""
    plist = TC.case_walkers("m", m)
    *_, out = run_chain("m", m, plist)
    check_chain("m", m, plist, out, f"m={m}")


@pytest.mark.parametrize("nf", TC.BATCH_NFS)
def test_transform_batch_sizes_and_bit_identity(nf):
    """B = 1, 2, 3, 5, 33, 64 (walker chunks of 4 .. 32 with odd tails, the ping-pong's odd last walker) against the
    oracle; every walker alone gives the bits it gets inside every batch."""
    walkers = TC.walkers(max(TC.BATCHES), far=True)
    do = case_device("nf", nf)
    alone = []
    for b, p in enumerate(walkers):
        md, rows = pack_rows(do, [p])
        alone.append(do.transform(md, rows))
    for B in TC.BATCHES:
        plist = walkers[:B]
        md, rows = pack_rows(do, plist)
        out = do.transform(md, rows)
        check_chain("nf", nf, plist, out, f"nf={nf} B={B}")
        for b in range(B):
            for k in ("flux", "X", "resid", "log_scale"):
                np.testing.assert_array_equal(out[k][b], alone[b][k][0], err_msg=f"nf={nf} B={B} walker {b} {k}")
    do.release_workspace()


@pytest.mark.parametrize("n", TC.RENORM_PIXELS)
def test_transform_renormalised_scale(n):
    """No log_scale: the scale is the ratio of two trapezoid sums reduced over the block (2, 3 and 257 pixels)."""
    plist = TC.case_walkers("pixels", n)
    *_, out = run_chain("pixels", n, plist)
    check_chain("pixels", n, plist, out, f"n={n}")


def test_transform_renormalised_scale_large_order():
    plist = TC.walkers(4, far=True, log_scale=False)
    *_, out = run_chain("nf", 16384, plist)
    check_chain("nf", 16384, plist, out, "nf=16384 renorm")


@pytest.mark.parametrize("variant", TC.MODEL_VARIANTS)
def test_transform_model_variants(variant):
    """Chebyshev off / three coefficients, extinction off / on, no Doppler shift, no broadening (static spline)."""
    plist = TC.walkers(4, **TC.variant_kw(variant))
    *_, out = run_chain("nf", 1024, plist)
    check_chain("nf", 1024, plist, out, variant)


# ------------------------------------------------------------------------------------------------ limits
def test_vsini_rejected_outside_the_fft_limits_before_any_launch():
    """nf = 8 (too few 16-point blocks for the spline fit) and nf = 131072 (beyond the broadening's transform): every
    entry point refuses a model with vsini up front, naming both limits; the same contexts serve models without vsini."""
    small = synth.make_order(N=6, m=4, seed=3, pad=0.04)
    assert len(small["emu_wl"]) == 8
    big = TC.make_nf_order(131072, N=600, pad_steps=33000, seed=4)
    for o, nf in ((small, 8), (big, 131072)):
        oo = TC.oracle_order(o)
        do = device_order(oo)
        assert do.nf == nf
        bad = TC.walkers(2, log_scale=True)
        md = do.model_desc(True, True, True, False, 0, 2)
        for call in (lambda: do.param_stride(md), lambda: do.transform(md, np.zeros((2, 6 + do.P + 2))),
                     lambda: do.loglike(md, np.zeros((2, 6 + do.P + 2)))):
            with pytest.raises(_lib.StarfishAMDError, match=r"16 <= nf <= 65536"):
                call()
        assert do.workspace_bytes(md, 2) == 0
        good = [dict(p) for p in bad]
        for p in good:
            del p["vsini"]
        md_good, rows = pack_rows(do, good)
        out = do.transform(md_good, rows)
        for b, p in enumerate(good):
            r = TC.chain_reference(oo, p)
            assert out["info"][b] == 0
            assert np.all(np.abs(out["flux"][b] - r["flux"]) <= r["tol_flux"]), (nf, b)
            assert np.all(np.abs(out["X"][b] - r["X"]) <= r["tol_X"]), (nf, b)
        if nf == 8:
            lnl = do.loglike(md_good, rows)
            for b, p in enumerate(good):
                want = O.log_likelihood(oo, p)
                assert lnl["info"][b] == 0 and abs(lnl["lnl"][b] - want) <= 1e-8 * abs(want) + 1e-8
            # a multi-order call whose second segment cannot take the model is refused as a whole
            o2 = TC.make_nf_order(64, seed=5)
            do2 = device_order(TC.oracle_order(o2))
            md2, rows2 = pack_rows(do2, bad)
            with pytest.raises(_lib.StarfishAMDError, match=r"16 <= nf <= 65536"):
                D.loglike_multi([do2, do], md2, [rows2, rows2])
        do.release_workspace()


# ------------------------------------------------------------------------------------------------ free functions
FREE_NFS = (4, 8, 16, 16384, 32768, 65536)
FREE_ROWS = (1, 3, 40)


@functools.lru_cache(maxsize=None)
def free_rows(nf, rows):
    w = 5000.0 * np.exp(np.arange(nf) * TC.DV / synth.C_KMS)
    rng = np.random.default_rng(nf + rows)
    f = 1 + 0.1 * np.sin(w / 7)[None, :] + 0.05 * rng.standard_normal((rows, nf))
    return w, f


@pytest.mark.parametrize("nf", FREE_NFS)
def test_free_broadening(nf):
    """rotational_broaden / instrumental_broaden (the full-length transform: LDS up to 8192, global scratch beyond,
    one scratch row per input row) against the oracle, 1, 3 and 40 rows."""
    for rows in FREE_ROWS:
        w, f = free_rows(nf, rows)
        for vsini in (0.5, 30.0, 300.0):
            want, tol = TC.broaden_reference(w, f, "rot", vsini)
            got = T.rotational_broaden(w, f if rows > 1 else f[0], vsini)
            err = np.abs(np.atleast_2d(got) - want) / tol
            assert err.max() <= 1, (nf, rows, vsini, float(err.max()))
        for fwhm in (0.0, TC.kill_fwhm(nf, O.min_velocity_step(w))):
            want, tol = TC.broaden_reference(w, f, "inst", fwhm)
            got = T.instrumental_broaden(w, f if rows > 1 else f[0], fwhm)
            err = np.abs(np.atleast_2d(got) - want) / tol
            assert err.max() <= 1, (nf, rows, fwhm, float(err.max()))


# ------------------------------------------------------------------------------------------------ resample
RES_NS = (6, 7, 63, 64, 65, 128, 129, 1000)
RES_ROWS = (1, 3, 64, 65, 130)


def source_grid(n, jitter):
    rng = np.random.default_rng(n)
    step = np.full(n - 1, 2.0 / synth.C_KMS)
    if jitter:
        step = step * (1 + 0.3 * rng.uniform(-1, 1, n - 1))
    return 5000.0 * np.exp(np.concatenate([[0.0], np.cumsum(step)]))


def queries(x):
    """Data points, interior knots, both ends, up to two spacings outside either end, a shuffled mix of all of them."""
    rng = np.random.default_rng(len(x))
    h0, h1 = x[1] - x[0], x[-1] - x[-2]
    ends = [x[0], x[-1], x[0] - 2 * h0, x[0] - 0.7 * h0, x[-1] + 0.4 * h1, x[-1] + 2 * h1]
    mid = x[:-1] + np.diff(x) * rng.uniform(0, 1, len(x) - 1)
    q = np.concatenate([x, O.quintic_knots(x)[6:-6], ends, mid])
    return np.concatenate([q, rng.permutation(q)])


@pytest.mark.parametrize("jitter", [False, True], ids=["loguniform", "jitter30"])
@pytest.mark.parametrize("n", RES_NS)
def test_resample(n, jitter):
    """k = 5 interpolating spline (k_spline_solve in 64-lane waves, one lane per row) against FITPACK."""
    x = source_grid(n, jitter)
    xq = queries(x)
    assert np.any(xq < x[0]) and np.any(xq > x[-1]) and not np.all(np.diff(xq) > 0)
    rng = np.random.default_rng(100 + n)
    for rows in RES_ROWS:
        y = 1 + 0.1 * np.sin(x / 3)[None, :] + 0.05 * rng.standard_normal((rows, n))
        got = np.atleast_2d(T.resample(x, y if rows > 1 else y[0], xq))
        want = np.atleast_2d(O.quintic_resample(x, y, xq))
        tol = TC.resample_tol(x, y, xq)
        err = np.abs(got - want) / tol[None, :]
        assert err.max() <= 1, (n, jitter, rows, float(err.max()), np.unravel_index(err.argmax(), err.shape))
        empty = T.resample(x, y, np.zeros(0))
        assert empty.shape == (rows, 0)


def test_resample_rejects_short_and_non_increasing_grids():
    x = source_grid(7, False)
    with pytest.raises(_lib.StarfishAMDError, match="at least 6"):
        T.resample(x[:5], np.ones(5), x[:3])
    for bad in (x[::-1].copy(), np.concatenate([x[:3], x[2:6]])):
        with pytest.raises(_lib.StarfishAMDError, match="strictly increasing"):
            T.resample(bad, np.ones(len(bad)), x[:3])


# ------------------------------------------------------------------------------------------------ end to end
def close_lnl(got, want):
    return abs(got - want) <= 1e-8 * abs(want) + 1e-8


def test_loglike_at_nf_16384():
    """The dense likelihood (default sequence) of an order whose transform is the largest one kept in LDS."""
    o = TC.make_nf_order(16384, N=3000, pad_steps=3000, seed=8)
    oo = TC.oracle_order(o)
    do = device_order(oo)
    plist = [synth.vector_to_oracle_params(v) for v in synth.walker_ball(o, B=4, seed=3)]
    md, rows = pack_rows(do, plist)
    out = do.loglike(md, rows)
    for b, p in enumerate(plist):
        want = O.log_likelihood(oo, p)
        assert out["info"][b] == 0 and close_lnl(out["lnl"][b], want), (b, out["lnl"][b], want)
    do.release_workspace()


def test_echelle_orders_of_different_fft_length():
    """Orders of nf 2048, 16384 and 32768 in one multi-order call (the transient buffers sized by the largest nf,
    every order transforming at its own), order by order against the oracle."""
    spec = ((2048, 600), (16384, 4000), (32768, 10000))
    orders = [TC.make_nf_order(nf, N=600, pad_steps=ps, seed=70 + i, wave0=5000.0 * 1.02**i)
              for i, (nf, ps) in enumerate(spec)]
    em = synth.build_echelle(orders)
    P = synth.shared_ball(orders[0], B=4, seed=11)
    total, per_order = em.log_likelihood_batch(P, return_orders=True)
    for i, o in enumerate(orders):
        oo = TC.oracle_order(o)
        want = np.array([O.log_likelihood(oo, synth.shared_to_oracle_params(o, p)) for p in P])
        assert all(close_lnl(g, w) for g, w in zip(per_order[i], want)), (spec[i], per_order[i], want)
    np.testing.assert_allclose(total, per_order.sum(axis=0), rtol=1e-14)
