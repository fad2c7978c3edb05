"""The Fisher information of the covariance hyper-parameters in numpy, F_ij = 1/2 tr(C^-1 D_i C^-1 D_j) with D_i = dC / d theta_i
(tests/cov_derivatives.py), and the size its rounding-error bounds are measured against.  A helper of
tests/test_cov_fisher_host.py and tests/test_gpu_cov_fisher.py, not a test.  The longdouble Cholesky factor and inverse are those
of tests/test_gpu_gradient.py, restated."""
import numpy as np

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


def contract(W, D_list):
    """1/2 sum_ab (W D_j W)_ab (D_i)_ab for every pair of the list: (s, s)."""
    S = [W @ D @ W for D in D_list]
    s = len(D_list)
    F = np.zeros((s, s), dtype=W.dtype)
    for i in range(s):
        for j in range(s):
            F[i, j] = 0.5 * np.sum(D_list[i] * S[j])
    return F


def fisher_cov(C, D_list, dtype=LD):
    """1/2 tr(C^-1 D_i C^-1 D_j) in ``dtype`` (np.longdouble or np.float64): (s, s)."""
    return contract(cinv(C, dtype), [np.asarray(D).astype(dtype) for D in D_list])


def size(Cinv, Dbar_list):
    """1/2 sum (|C^-1| Dbar_i |C^-1|) o Dbar_j with Dbar from cov_derivatives.slot_derivatives(absolute=True): what a rounding
    error of an entry of F is measured against.  float64, (s, s)."""
    return contract(np.abs(np.asarray(Cinv)).astype(np.float64), [np.asarray(D, dtype=np.float64) for D in Dbar_list])
