"""The inputs of test_gpu_potrf_contract.py are what they claim (CPU only): A = L0 L0^T is exact, LAPACK returns L0 and
reports every planted pivot failure at its column, the poisoned layouts are poisoned where they should be, and the GPU
tests' tolerance separates a correct factorisation from one that lost a single 16-wide K chunk of a single tile update."""
import numpy as np
import pytest
from scipy.linalg.lapack import dpotrf

import potrf_cases as PC

GPU_ATOL = 1e-12  # |L - L0| entrywise in test_gpu_potrf_contract.py


@pytest.mark.parametrize("n,batch", PC.SHAPES)
def test_inputs_are_exact_and_lapack_returns_the_known_factor(n, batch):
    L0, A = PC.case(n, batch)
    assert L0.shape == A.shape == (batch, n, n)
    k = L0 * PC.Q
    assert np.array_equal(k, np.round(k)) and np.array_equal(L0, np.tril(L0))
    off = np.tril(k, -1)
    d = np.diagonal(k, axis1=1, axis2=2)
    assert np.abs(off).max() <= PC.OFF_RANGE and d.min() >= PC.Q and d.max() <= 4 * PC.Q
    rows = sorted({0, 1, 63, n // 2, n - 2, n - 1})
    for b in range(batch):
        Lq = L0[b].astype(np.longdouble)
        for r in rows:
            want = (Lq[r][None, :] * Lq).sum(axis=1)
            assert np.array_equal(A[b, r].astype(np.longdouble), want), (b, r)  # bit for bit
        assert np.array_equal(A[b], A[b].T)
        c, info = dpotrf(A[b], lower=1)
        assert info == 0
        assert np.abs(np.tril(c) - L0[b]).max() <= 1e-14


@pytest.mark.parametrize("n", sorted(PC.PIVOTS))
def test_lapack_reports_every_planted_pivot(n):
    L0, A = PC.case(n, PC.PIVOT_BATCH)
    assert sorted(p for pair in PC.pivot_pairs(n) for p in pair) == sorted(PC.PIVOTS[n])
    for b in (1, 4):
        for p in PC.PIVOTS[n]:
            bad = PC.not_pd_at(A[b], L0[b], p)
            assert np.array_equal(bad - A[b], -(L0[b, p, p] ** 2 + 1.0) * np.outer(np.eye(n)[p], np.eye(n)[p]))
            _, info = dpotrf(bad, lower=1)
            assert info == p + 1, (b, p, info)


@pytest.mark.parametrize("n", [192, 320])
def test_embedded_layouts_are_poisoned_outside_the_lower_triangles(n):
    L0, A = PC.case(n, 3)
    for lay in PC.layouts(n):
        assert lay.lda >= n and lay.lda % 2 == 0 and lay.stride % 2 == 0 and lay.stride >= (n - 1) * lay.lda + n
        for upper in ("sym", "nan"):
            e = PC.embed(A, lay, upper=upper)
            assert e.front >= 64 * (lay.lda + 1) and e.front % 2 == 0
            assert e.buf.size - (e.front + 3 * lay.stride) >= 64 * lay.lda + 4096
            assert np.isnan(e.buf[:e.front]).all() and np.isnan(e.buf[e.front + 2 * lay.stride + (n - 1) * lay.lda + n:]).all()
            assert e.outside_is_nan(e.buf)
            M = e.matrices()
            assert np.array_equal(np.tril(M), np.tril(A))
            iu = np.triu_indices(n, 1)
            if upper == "nan":
                assert np.isnan(M[:, iu[0], iu[1]]).all()
            else:
                assert np.array_equal(M, A)
            # one written double anywhere outside the matrices is seen
            for pos in (0, e.front - 1, e.buf.size - 1) + ((e.front + n,) if lay.lda > n else ()) + (
                    (e.front + lay.stride - 1,) if lay.stride > n * lay.lda else ()):
                hit = e.buf.copy()
                hit[pos] = 0.0
                assert not e.outside_is_nan(hit), pos


def test_known_logdet_and_sqmah_of_the_solve_cases():
    L0, z0, R, logdet, sqmah = PC.solve_case(192, 3)
    for b in range(3):
        assert np.array_equal(R[b].astype(np.longdouble), (L0[b].astype(np.longdouble) * z0[b].astype(np.longdouble)).sum(axis=1))
        z = np.linalg.solve(L0[b], R[b])
        np.testing.assert_allclose(z @ z, sqmah[b], rtol=1e-11)
        np.testing.assert_allclose(np.linalg.slogdet(L0[b] @ L0[b].T)[1], logdet[b], rtol=1e-12)


def test_one_missing_k_chunk_is_a_million_tolerances_away():
    """n = 768, tile (5, 3): the emulation of the blocked algorithm agrees with L0 to rounding; with ONE 16-wide K chunk left out
    of that ONE tile update it misses L0 by more than 1e6 x the tolerance of the GPU tests."""
    n = 768
    L0, A = PC.case(n, 17)
    good = PC.blocked_cholesky(A[2])
    assert np.abs(good - L0[2]).max() <= 1e-13
    for chunk in (0, 7, 23):
        bad = PC.blocked_cholesky(A[2], skip=(5, 3, chunk))
        err = np.abs(bad - L0[2])
        assert err.max() > 1e6 * GPU_ATOL, (chunk, err.max())
        # ... and the damage starts in that tile: everything above and left of it is untouched
        assert np.abs(bad[:640] - L0[2][:640]).max() <= 1e-13 and np.abs(bad[640:, :384] - L0[2][640:, :384]).max() <= 1e-13
