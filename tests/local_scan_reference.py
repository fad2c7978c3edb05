"""The score scan for a new local kernel in numpy: quad = alpha^T k alpha, trace = tr(W k), fisher = 1/2 tr(W k W k) with W = C^-1,
alpha = W r and k = oracle.sf_oracle.gaussian_local(wave, 1.0, mu, sigma), and the sizes the rounding-error bounds are measured
against.  A helper of tests/test_local_scan_host.py and tests/test_gpu_local_scan.py, not a test.  The longdouble Cholesky factor
and inverse are those of tests/cov_fisher_reference.py, restated."""
import numpy as np

from oracle import sf_oracle as O

LD = np.longdouble


def cholesky_longdouble(A):
    L = np.zeros_like(A)
    for j in range(A.shape[0]):
        L[j, j] = np.sqrt(A[j, j] - L[j, :j] @ L[j, :j])
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def inverse_longdouble(L):
    X = np.zeros_like(L)
    for i in range(L.shape[0]):
        row = -(L[i, :i] @ X[:i])
        row[i] += 1
        X[i] = row / L[i, i]
    return X


def cinv(C, dtype=LD):
    """C^-1: in longdouble as X^T X with X the inverse of the longdouble Cholesky factor, in float64 by numpy.linalg.inv."""
    if dtype is np.float64 or dtype == np.float64:
        return np.linalg.inv(np.asarray(C, dtype=np.float64))
    X = inverse_longdouble(cholesky_longdouble(np.asarray(C).astype(LD)))
    return X.T @ X


def kernel(wave, mu, sigma):
    """k(mu, sigma): the matrix a local kernel of that centre and width (km/s) adds at amplitude 1 (float64, as the oracle has it)."""
    return O.gaussian_local(np.asarray(wave, dtype=np.float64), 1.0, float(mu), float(sigma))


def patch(wave, mu, sigma):
    """The pixels k lives on, as (lo, hi + 1); (0, 0) if there is none.  Everything outside is exactly zero in ``kernel``."""
    idx = np.nonzero(O.local_metric(wave, mu) <= 4 * sigma)[0]
    return (int(idx[0]), int(idx[-1]) + 1) if idx.size else (0, 0)


def patch_kernel(wave, mu, sigma):
    """(lo, hi, the block of ``kernel`` on the patch): the oracle's formula on the patch's own wavelengths gives the same
    entries, and every entry of ``kernel`` outside the block is zero (tests/test_local_scan_host.py checks both)."""
    lo, hi = patch(wave, mu, sigma)
    w = np.asarray(wave, dtype=np.float64)[lo:hi]
    return lo, hi, (O.gaussian_local(w, 1.0, float(mu), float(sigma)) if hi > lo else np.zeros((0, 0)))


def three(W, alpha, wave, mu, sigma):
    """(quad, trace, fisher) in the dtype of ``W`` and ``alpha`` (np.longdouble or np.float64), contracted on the patch alone
    (k is zero elsewhere, so nothing is left out)."""
    lo, hi, k = patch_kernel(wave, mu, sigma)
    k = k.astype(W.dtype)
    Wp, ap = W[lo:hi, lo:hi], alpha[lo:hi]
    M = Wp @ k
    return ap @ k @ ap, np.sum(Wp * k), 0.5 * np.sum(M * M.T)


def sizes(W, alpha, wave, mu, sigma):
    """size_quad = |alpha|^T k |alpha|, size_trace = sum |W| o k, size_fisher = 1/2 sum (|W| k |W|) o k (k >= 0): what the
    rounding error of each number is measured against.  float64."""
    lo, hi, k = patch_kernel(wave, mu, sigma)
    aW, aa = np.abs(np.asarray(W[lo:hi, lo:hi])).astype(np.float64), np.abs(np.asarray(alpha[lo:hi])).astype(np.float64)
    return aa @ k @ aa, np.sum(aW * k), 0.5 * np.sum((aW @ k @ aW) * k)


def scan(C, r, wave, cand, dtype=LD):
    """``three`` and ``sizes`` for every candidate row (mu, sigma) of ``cand``, from the matrix C (jitter included) and the
    residual r: (ncand, 3) in ``dtype`` and (ncand, 3) float64."""
    W = cinv(C, dtype)
    alpha = W @ np.asarray(r).astype(W.dtype)
    got = np.array([three(W, alpha, wave, mu, sg) for mu, sg in cand], dtype=W.dtype).reshape(-1, 3)
    size = np.array([sizes(W, alpha, wave, mu, sg) for mu, sg in cand], dtype=np.float64).reshape(-1, 3)
    return got, size
