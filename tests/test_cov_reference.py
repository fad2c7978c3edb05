"""CPU checks of the references behind tests/test_gpu_cov_structure.py: the restricted evaluation of the structured
kernels gives the oracle's bits, the banded-Woodbury likelihood (the reference above N = 32 768, where no dense matrix
fits) matches the dense oracle, the grids are what they claim to be."""
import numpy as np
import pytest

import cov_cases as CC
from oracle import sf_oracle as O
from starfish_amd import synth


@pytest.mark.parametrize("kind", ["A", "G", "L", "N"])
def test_dense_cov_is_the_oracle_bit_for_bit(kind):
    o = CC.make_grid_order("G3", 700, m=5, seed=3)
    oo = CC.oracle_order_of(o)
    for p in CC.batch(o, kind):
        flux, cov, scale = CC.dense_cov(oo, p)
        f0, c0, s0 = O.forward_model(oo, p)
        np.testing.assert_array_equal(cov, c0)
        np.testing.assert_array_equal(flux, f0)
        assert scale == s0
        lnl, logdet, sqmah = CC.dense_loglike(oo, flux, cov)
        want = O.log_likelihood(oo, p, return_parts=True)
        assert (lnl, logdet, sqmah) == tuple(want[:3])


@pytest.mark.parametrize("grid,kind", [("G1", "A"), ("G2", "G"), ("G3", "A"), ("G3", "L"), ("G5", "A")])
def test_band_woodbury_matches_the_dense_oracle(grid, kind):
    o = CC.make_grid_order(grid, 3000)
    oo = CC.oracle_order_of(o)
    for p in CC.batch(o, kind):
        hw = CC.support_halfwidth(oo, p)
        assert 0 <= hw < 3000 // 4
        lnl, logdet, sqmah = CC.band_woodbury(oo, p, hw)
        flux, cov, _ = CC.dense_cov(oo, p)
        _, ld0, sq0 = CC.dense_loglike(oo, flux, cov)
        assert abs(logdet - ld0) <= 1e-12 * abs(ld0), (logdet, ld0)
        assert abs(sqmah - sq0) <= 1e-10 * abs(sq0), (sqmah, sq0)
        if hw:
            with pytest.raises(AssertionError, match="wider than the band"):
                CC.band_woodbury(oo, p, hw - 1)  # the reference refuses a band its support does not fit


def test_band_woodbury_of_the_plain_oracle():
    """One walker straight through O.log_likelihood (no restricted kernels in between)."""
    o = CC.make_grid_order("G1", 1000, m=3, seed=4)
    oo = CC.oracle_order_of(o)
    p = CC.batch(o, "A", n_local=6)[1]
    _, ld0, sq0, _ = O.log_likelihood(oo, p, return_parts=True)
    _, logdet, sqmah = CC.band_woodbury(oo, p, CC.support_halfwidth(oo, p))
    assert abs(logdet - ld0) <= 1e-12 * abs(ld0)
    assert abs(sqmah - sq0) <= 1e-10 * abs(sq0)


def test_grids():
    for n in (2240, 3000, 4096):
        g = {k: CC.make_grid_order(k, n)["wave"] for k in CC.GRIDS}
        assert all(len(w) == n for w in g.values())
        assert CC.q_spread(g["G1"]) <= CC.LOGUNIFORM_SPREAD
        assert CC.q_spread(g["G2"]) > 1e-3
        assert CC.q_spread(g["G3"]) > 0.9  # the gaps
        assert 1e-10 <= CC.q_spread(g["G5"]) <= CC.LOGUNIFORM_SPREAD
        assert not np.all(np.diff(g["G4"]) > 0)
    # the synthetic orders of the suite and the benchmark (dv = 2 and 4 km/s) stay on the library's table path (at
    # dv = 1 the rounding of the grid alone spreads the ratio by ~2.1e-10: those take the per-entry path)
    for dv in (2.0, 4.0):
        for wave0 in (3000.0, 5000.0, 10000.0):
            for n in (1024, 4096, 33000):
                w = wave0 * np.exp(np.arange(n) * dv / synth.C_KMS)
                assert CC.q_spread(w) <= CC.LOGUNIFORM_SPREAD, (dv, wave0, n)


def test_farthest_block_and_drop():
    n = 600
    S = np.zeros((n, n))
    S[450, 10] = S[10, 450] = 1e-3
    S[300, 290] = S[290, 300] = 1e-3
    assert CC.farthest_block(S) == (3, 0)
    assert CC.farthest_block(np.zeros((n, n))) is None
    cov = np.eye(n) * 1e-2 + S
    base = CC.drop_block_logdet(cov, np.zeros_like(S), (3, 0))
    assert CC.drop_block_logdet(cov, S, (3, 0)) > base  # removing the off-diagonal pair raises the determinant
