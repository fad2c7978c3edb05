"""Selected inversion on the band, restated in numpy for the tests: the entries of Sigma = A^-1 inside the band of a symmetric
positive definite band matrix, from its block Cholesky factor by Takahashi's recurrence over block columns from the last to
the first (blocks of 16, identity padding to whole blocks, nbr - 1 = max(2, (w + 31) // 16 - 1) blocks below the diagonal, as
the device's window).  With F_k = L_kk^-1, G_I = L_{k+1+I,k} F_k and cnt = min(nbr - 1, nblk - 1 - k):

    Sigma_{k+1+J,k} = - sum_{I < cnt} Sigma_{k+1+J,k+1+I} G_I        (J < cnt;  Sigma_{a,b} = Sigma_{b,a}^T for a < b)
    Sigma_{k,k}     = F_k^T F_k - sum_{I < cnt} G_I^T Sigma_{k+1+I,k}

Only blocks inside the block band are touched (the factor has no fill outside it), so the result is exact on the band.  Any
dtype numpy multiplies in: float64 and np.longdouble are used.  Also the entrywise bound the device's band is held to, and the
covariance gradient contracted over the band."""
import numpy as np
from scipy.linalg import solve_triangular

BB = 16
U = 2.0 ** -53
LD = np.longdouble


def gamma(k):
    return k * U / (1 - k * U)


def band_spd(rng, n, w):
    """(A, band, ldb): a dense symmetric positive definite matrix of half-bandwidth min(w, n - 1), strictly diagonally dominant,
    and its lower band storage band[i, d] = A[i, i - d] with w + 1 diagonals (zero beyond the matrix), ldb even."""
    A = np.zeros((n, n))
    for d in range(1, min(w, n - 1) + 1):
        A[np.arange(d, n), np.arange(n - d)] = rng.standard_normal(n - d) * 0.3
    A = A + A.T
    A[np.diag_indices(n)] = np.abs(A).sum(axis=1) + 0.5 + rng.random(n)
    return A, lower_band(A, w, w + 1 + (w + 1) % 2), w + 1 + (w + 1) % 2


def lower_band(A, w, ldb=None):
    """band[i, d] = A[i, i - d], 0 <= d <= min(i, w); zero elsewhere."""
    n = A.shape[0]
    band = np.zeros((n, ldb or w + 1), dtype=A.dtype)
    for d in range(min(w, n - 1) + 1):
        band[d:, d] = A[np.arange(d, n), np.arange(n - d)]
    return band


def cholesky(A):
    L = np.zeros_like(A)
    for j in range(A.shape[0]):
        L[j, j] = np.sqrt(A[j, j] - L[j, :j] @ L[j, :j])
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def inverse_lower(L):
    X = np.zeros_like(L)
    for i in range(L.shape[0]):
        row = -(L[i, :i] @ X[:i])
        row[i] += 1
        X[i] = row / L[i, i]
    return X


def selected_inverse(A, w, dtype=np.float64):
    """dict(band=(n, w + 1) with band[i, d] = (A^-1)[i, i - d], L=(n, n) the Cholesky factor) of the dense band matrix A with
    half-bandwidth <= w, everything in ``dtype``."""
    n = A.shape[0]
    nblk = -(-n // BB)
    npad, nb1 = nblk * BB, max(3, (w + 2 * BB - 1) // BB) - 1
    M = np.eye(npad, dtype=dtype)
    M[:n, :n] = A
    L = np.zeros((npad, npad), dtype=dtype)
    blk = lambda X, a, b: X[a * BB:(a + 1) * BB, b * BB:(b + 1) * BB]  # noqa: E731
    F = []
    for k in range(nblk):  # the block factor, right-looking, inside the block band
        cnt = min(nb1, nblk - 1 - k)
        blk(L, k, k)[:] = cholesky(blk(M, k, k))
        F.append(inverse_lower(blk(L, k, k)))
        for i in range(cnt):
            blk(L, k + 1 + i, k)[:] = blk(M, k + 1 + i, k) @ F[k].T
        for i in range(cnt):
            for j in range(i + 1):
                blk(M, k + 1 + i, k + 1 + j)[:] -= blk(L, k + 1 + i, k) @ blk(L, k + 1 + j, k).T
    S = {}
    for k in reversed(range(nblk)):
        cnt = min(nb1, nblk - 1 - k)
        G = [blk(L, k + 1 + i, k) @ F[k] for i in range(cnt)]
        for j in range(cnt):
            acc = np.zeros((BB, BB), dtype=dtype)
            for i in range(cnt):
                a, b = k + 1 + j, k + 1 + i
                acc = acc - (S[a, b] if a >= b else S[b, a].T) @ G[i]
            S[k + 1 + j, k] = acc
        d = F[k].T @ F[k]
        for i in range(cnt):
            d = d - G[i].T @ S[k + 1 + i, k]
        S[k, k] = np.tril(d) + np.tril(d, -1).T  # (read from either side later: mirrored from its lower triangle)
    band = np.zeros((n, w + 1), dtype=dtype)
    for (a, b), s in S.items():
        i, j = np.meshgrid(np.arange(a * BB, (a + 1) * BB), np.arange(b * BB, (b + 1) * BB), indexing="ij")
        ok = (i < n) & (i - j >= 0) & (i - j <= w)
        band[i[ok], (i - j)[ok]] = s[ok]
    return dict(band=band, L=L[:n, :n])


def band_of(X, w):
    """The lower band of a dense symmetric matrix in the layout of selected_inverse()["band"]."""
    return lower_band(X, w)


def on_band(n, w):
    """Mask of the entries of an (n, w + 1) band that belong to the matrix: d <= i."""
    return np.arange(w + 1)[None, :] <= np.arange(n)[:, None]


def selinv_bound(A, w, L):
    """The entrywise bound of a float64 selected inversion of A (half-bandwidth <= w) on the band, (n, w + 1), from the
    reference factor L alone (rounded to float64; the products of the bound itself are float64).  With Xl = L^-1, X = A^-1:
        (|X| dA |X|)_ij + gamma_2n (E + E^T)_ij + gamma_{n+1} (|Xl|^T |Xl|)_ij,
        dA = 1e-13 |A| + gamma_{w+17} |L||L|^T         (the band factor: sums of at most w + 16 products per entry)
        E = |Xl|^T |Xl||L||Xl|                         (tests/test_gpu_potri_blocks.py: the inverse from the factor)"""
    n = A.shape[0]
    L64 = np.asarray(L, dtype=np.float64)
    aL = np.abs(L64)
    Xl = solve_triangular(L64, np.eye(n), lower=True)
    aXl = np.abs(Xl)
    aX = np.abs(Xl.T @ Xl)
    dA = 1e-13 * np.abs(A) + gamma(w + 17) * (aL @ aL.T)
    E = aXl.T @ (aXl @ (aL @ aXl))
    return band_of(aX @ dA @ aX + gamma(2 * n) * (E + E.T) + gamma(n + 1) * (aXl.T @ aXl), w)


def banded_cov_gradient(q, D, w, dtype=LD):
    """1/2 sum_{ij on the band} (alpha_i alpha_j - Sigma_ij + (Vs Vs^T)_ij) D_ij for every (label, D) of ``D``
    (tests/cov_derivatives.slot_derivatives), from the pieces ``q`` of tests/banded_derivatives.pieces: Sigma = Bd^-1 by
    selected_inverse, T = Bd^-1 [r, Y^T] from the same factor, S = I + Y T_Y = L_S L_S^T, Vs = T_Y L_S^-T,
    alpha = (Sigma - Vs Vs^T) r = t_r - Vs L_S^-1 g with g = Y t_r.  Off-diagonal entries of the lower band count twice."""
    n = len(q["r"])
    sel = selected_inverse(q["Bd"].astype(dtype), w, dtype)
    L = sel["L"]
    Lw = cholesky(q["S"].astype(dtype))
    Y = solve_lower(Lw, q["X"].astype(dtype))
    rhs = np.column_stack([q["r"].astype(dtype), Y.T])
    T = solve_lower(L, solve_lower(L, rhs), transpose=True)
    gram = rhs.T @ T
    m = Y.shape[0]
    Ls = cholesky(np.eye(m, dtype=dtype) + gram[1:, 1:])
    Vs = T[:, 1:] @ inverse_lower(Ls).T
    alpha = T[:, 0] - Vs @ solve_lower(Ls, gram[1:, 0])
    Aband = band_of(np.outer(alpha, alpha) + Vs @ Vs.T, w) - sel["band"]
    Aband[:, 1:] *= 2
    Aband[~on_band(n, w)] = 0
    return [(label, 0.5 * np.sum(Aband * band_of(np.asarray(d, dtype=dtype), w))) for label, d in D]


def solve_lower(L, B, transpose=False):
    """L^-1 B, or L^-T B, by substitution in L's dtype."""
    n = L.shape[0]
    X = np.array(B, dtype=L.dtype)
    if not transpose:
        for i in range(n):
            X[i] = (X[i] - L[i, :i] @ X[:i]) / L[i, i]
    else:
        for i in reversed(range(n)):
            X[i] = (X[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
    return X
