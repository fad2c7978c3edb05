"""Covariance fill and likelihood across covariance structure, wavelength grid and emulator rank.

The likelihood materialises only the 128 x 128 tiles that k_tile_map flags for a walker, the dense fill of
sf_forward_batch / sf_cov_fill_batch culls with sf_block_support: a tile either map misses loses its K_global / K_local
part without an error.  These cases leave the walker ball of synth.centre_params (a 60 km/s band next to the diagonal,
one local kernel, constant sigma, m = 4 or 8): bands that reach a tile through its corner only, narrower than a pixel,
32 local kernels on tile boundaries and outside the array, unsorted / masked / nearly log-uniform grids, m from 1 to
32, N above 32 768.  Every likelihood case first proves that it could see a dropped tile (the sensitivity check of
tests/cov_cases.py).  Needs an MI355X: run with -m gpu."""
import functools

import numpy as np
import pytest

import cov_cases as CC
from gpu_helpers import device_order, oracle_order, pack_rows
from oracle import sf_oracle as O
from starfish_amd import _device as D
from starfish_amd import _lib, synth

pytestmark = pytest.mark.gpu

NS = (2240, 3000, 4096)  # 64 mod 128 (shifted frame, wide sequence reachable), not a multiple of 64, a power of two
MS = (1, 3, 5, 8, 12, 17, 32)  # mpad 4, 4, 8, 8, 12, 20, 32

# (grid, N, m, batch kind): 'A' global + 32 locals, 'G' global only, 'L' 32 locals only, 'N' nothing structured
CASES = [(g, n, 8, "A") for g in CC.GRIDS for n in NS]
CASES += [(g, 3000, 8, k) for g in CC.GRIDS for k in ("G", "L", "N")]
CASES += [("G1", n, m, "A") for m in MS if m != 8 for n in (2240, 3000)]
SEQ_CASES = [("G1", 3000, m, "A") for m in (5, 12, 17)] + [("G3", 2240, 8, "A"), ("G4", 3000, 8, "L")]


def case_id(c):
    return f"{c[0]}-N{c[1]}-m{c[2]}-{c[3]}"


def close_lnl(got, want):
    return abs(got - want) <= 1e-8 * abs(want) + 1e-8


@functools.lru_cache(maxsize=None)
def order_of(grid, n, m):
    o = CC.make_grid_order(grid, n, m=m)
    oo = CC.oracle_order_of(o)
    return o, oo, device_order(oo)


@functools.lru_cache(maxsize=None)
def oracle_parts(case):
    """Per walker (lnl, logdet, sqmah) of the oracle, after the sensitivity check."""
    grid, n, m, kind = case
    o, oo, _ = order_of(grid, n, m)
    plist = CC.batch(o, kind)
    parts = []
    for p in plist:
        flux, cov, _ = CC.dense_cov(oo, p)
        lnl, logdet, sqmah = CC.dense_loglike(oo, flux, cov)  # (raises unless the oracle's matrix is positive definite)
        S = CC.structured_part(oo, p)
        blk = CC.farthest_block(S)
        if kind == "N":
            assert blk is None
        else:
            # a case that could not see its farthest structured tile dropped is a bug of the case
            assert blk is not None
            dropped = CC.drop_block_logdet(cov, S, blk)
            assert abs(dropped - logdet) > 100 * CC.LOGDET_RTOL * abs(logdet), (case, blk, dropped, logdet)
        parts.append((lnl, logdet, sqmah))
    return plist, parts


def check_loglike(out, parts, where=""):
    for b, (lnl, logdet, sqmah) in enumerate(parts):
        assert out["info"][b] == 0, (where, b, out["info"])
        assert abs(out["logdet"][b] - logdet) <= CC.LOGDET_RTOL * abs(logdet), (where, b, out["logdet"][b], logdet)
        assert abs(out["sqmah"][b] - sqmah) <= CC.SQMAH_RTOL * abs(sqmah), (where, b, out["sqmah"][b], sqmah)
        assert close_lnl(out["lnl"][b], lnl), (where, b, out["lnl"][b], lnl)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_loglike_forward_fill_banded(case):
    """Dense likelihood (automatic sequence), the whole forward covariance, both fills and the banded solver against
    the oracle for one batch of three walkers with different tile maps."""
    grid, n, m, kind = case
    o, oo, do = order_of(grid, n, m)
    plist, parts = oracle_parts(case)
    md, rows = pack_rows(do, plist)
    check_loglike(do.loglike(md, rows), parts, "dense")

    fwd = do.forward(md, rows)
    assert (fwd["info"] == 0).all(), fwd["info"]
    for b, p in enumerate(plist):
        _, cov, _ = CC.dense_cov(oo, p)
        np.testing.assert_allclose(fwd["cov"][b], cov, rtol=1e-10, atol=1e-11 * np.abs(cov).max())
    for lower in (True, False):
        got, info = do.cov_fill(md, rows, lower_only=lower)
        assert (info == 0).all(), info
        for b in range(len(plist)):
            want = fwd["cov"][b]
            tol = dict(rtol=1e-10, atol=1e-11 * np.abs(want).max())
            if lower:
                np.testing.assert_allclose(np.tril(got[b]), np.tril(want), **tol)
            else:
                np.testing.assert_allclose(got[b], want, **tol)

    # banded: every walker matches or is flagged (never silently wrong); the automatic solver recovers the flagged ones
    band = do.loglike(md, rows, solver="banded")
    flagged = band["info"] == D.INFO_BANDWIDTH
    assert np.all((band["info"] == 0) | flagged), band["info"]
    if kind != "N" and grid == "G4":
        assert flagged.all()  # unsorted wavelengths: no band exists
    check_loglike({k: v[~flagged] for k, v in band.items()}, [q for q, f in zip(parts, flagged) if not f], "banded")
    if flagged.any():
        check_loglike(do.loglike(md, rows, solver="auto"), parts, "auto")


@pytest.mark.parametrize("case", SEQ_CASES, ids=case_id)
def test_loglike_every_sequence(case, chol_sequence):
    grid, n, m, kind = case
    _, _, do = order_of(grid, n, m)
    plist, parts = oracle_parts(case)
    md, rows = pack_rows(do, plist)
    check_loglike(do.loglike(md, rows), parts, chol_sequence)


def test_loglike_multi_segments_of_different_n():
    """Two grids of different N (G1 at 2240, G2 at 3000) as the segments of one call: each segment matches the oracle
    and its own single-order call."""
    segs = [("G1", 2240, 8, "A"), ("G2", 3000, 8, "A")]
    devs, rows_list, parts_list = [], [], []
    for case in segs:
        _, _, do = order_of(*case[:3])
        plist, parts = oracle_parts(case)
        md, rows = pack_rows(do, plist)
        devs.append(do)
        rows_list.append(rows)
        parts_list.append(parts)
    outs = D.loglike_multi(devs, md, rows_list)
    for do, rows, parts, out in zip(devs, rows_list, parts_list, outs):
        check_loglike(out, parts, "multi")
        single = do.loglike(md, rows)
        np.testing.assert_allclose(out["lnl"], single["lnl"], rtol=1e-12)


# ------------------------------------------------------------------------------------------------ limits
def small_order(m=4, n=512):
    o = synth.make_order(N=n, m=m, seed=11)
    oo = oracle_order(o)
    return o, oo


def test_32_local_kernels_and_m_32_work():
    o, oo = small_order(m=32)
    do = device_order(oo)
    plist = CC.batch(o, "L", n_local=32)
    md, rows = pack_rows(do, plist)
    out = do.loglike(md, rows)
    for b, p in enumerate(plist):
        lnl, logdet, sqmah, _ = O.log_likelihood(oo, p, return_parts=True)
        check_loglike({k: v[b : b + 1] for k, v in out.items()}, [(lnl, logdet, sqmah)], "m=32, 32 locals")


def test_33_local_kernels_are_rejected():
    o, oo = small_order()
    do = device_order(oo)
    good = CC.batch(o, "A", n_local=32)
    md_good, rows_good = pack_rows(do, good)
    want = do.loglike(md_good, rows_good)
    assert (want["info"] == 0).all()

    bad = [dict(p, local_cov=p["local_cov"] + [p["local_cov"][-1]]) for p in good]
    md = do.model_desc(True, True, True, True, 33, 2)
    with pytest.raises(_lib.StarfishAMDError, match="SF_MAX_LOCAL"):
        do.param_stride(md)
    # rows in the C-ABI layout written by hand (pack_rows asks the library for the stride)
    stride = 6 + do.P + 2 + 3 * 33
    rows = np.zeros((len(bad), stride))
    rows[:, : rows_good.shape[1] - 3] = rows_good[:, :-3]
    rows[:, 6 + do.P + 2 :] = np.array([np.ravel(p["local_cov"]) for p in bad])
    with pytest.raises(_lib.StarfishAMDError, match="SF_MAX_LOCAL"):
        do.loglike(md, rows)
    with pytest.raises(_lib.StarfishAMDError, match="SF_MAX_LOCAL"):
        do.forward(md, rows)
    with pytest.raises(_lib.StarfishAMDError, match="SF_MAX_LOCAL"):
        do.loglike(md, rows, solver="banded")
    again = do.loglike(md_good, rows_good)
    np.testing.assert_array_equal(again["lnl"], want["lnl"])

    params = dict(synth.centre_params(o))
    params["local_cov"] = [dict(mu=mu, log_amp=la, log_sigma=ls) for mu, la, ls in bad[0]["local_cov"]]
    with pytest.raises(_lib.StarfishAMDError, match="SF_MAX_LOCAL"):
        synth.build_model(o, params=params).log_likelihood()
    again = do.loglike(md_good, rows_good)
    np.testing.assert_array_equal(again["lnl"], want["lnl"])


def test_m_33_is_rejected_by_ctx_create():
    o = synth.make_order(N=256, m=33, seed=12)
    oo = oracle_order(o)
    with pytest.raises(_lib.StarfishAMDError, match="SF_MAX_M"):
        device_order(oo)
    o4, oo4 = small_order(n=256)
    do = device_order(oo4)
    p = synth.vector_to_oracle_params(synth.centre_vector(o4))
    md, rows = pack_rows(do, [p])
    out = do.loglike(md, rows)
    assert out["info"][0] == 0 and close_lnl(out["lnl"][0], O.log_likelihood(oo4, p))


# ------------------------------------------------------------------------------------------------ N > 32 768
def big_case():
    """N = 33 000 (129 + 129 tile rows of 128, 258 in all) with a varying sigma, two walkers of narrow structure
    whose local kernels sit in the last two tile rows as well as at the start."""
    N = 33000
    o = dict(synth.make_order(N=N, m=4, seed=21))
    x = np.linspace(0, 1, N)
    o["sigma"] = 0.01 + 0.004 * np.sin(2 * np.pi * 3 * x) + 0.002 * np.cos(2 * np.pi * 7 * x + 1)
    oo = oracle_order(o)
    w = o["wave"]
    plist = []
    for k, (px, lsig) in enumerate(((40, 12.0), (24, 20.0))):
        p = CC.base_params(k)
        p["global_cov"] = CC.global_reaching(w, px, -6.0 + 0.3 * k)
        p["local_cov"] = [(float(w[32900 - 50 * k]), -5.5, float(np.log(lsig))),
                          (float(w[32800 + 60 * k]), -6.0, float(np.log(8.0))),
                          (float(w[100 + 30 * k]), -6.0, float(np.log(10.0)))]
        plist.append(p)
    return o, oo, plist


def test_loglike_above_32768_rows():
    """The likelihood's tile list held (tm << 8 | tn) in 16 bits: tile rows 256 and 257 (N > 32 768) wrapped to rows 0
    and 1, their tiles were never written and the factorisation read whatever the workspace held.  Two calls with the
    walkers swapped: the second one would see the first one's matrices there."""
    o, oo, plist = big_case()
    do = device_order(oo)
    ref = []
    for p in plist:
        hw = CC.support_halfwidth(oo, p)
        lnl, logdet, sqmah = CC.band_woodbury(oo, p, hw)
        _, dropped, _ = CC.band_woodbury(oo, p, hw, drop_rows_from=256 * CC.TILE)
        assert abs(dropped - logdet) > 100 * CC.LOGDET_RTOL * abs(logdet)  # the last tile rows matter
        ref.append((lnl, logdet, sqmah))
    md, rows = pack_rows(do, plist)
    check_loglike(do.loglike(md, rows), ref, "first call")
    check_loglike(do.loglike(md, rows[::-1].copy()), ref[::-1], "walkers swapped")
    do.release_workspace()
