"""numpy reference of the emulator training likelihood's gradient, in float64 or np.longdouble (helper of
tests/test_emulator_gradient_host.py and tests/test_gpu_emulator_gradient.py).

    V = iPhiPhi / lambda_xi + blockdiag_c K_c,   K_c[g,h] = variance_c exp(-1/2 sum_p ((x_gp - x_hp) / l_cp)^2)
    lnL = -1/2 (log det V + w^T V^-1 w),   d lnL / d theta = 1/2 sum_ij (alpha alpha^T - V^-1)_ij (dV / d theta)_ij

`row` is a hyper-parameter vector in the units and the order of Emulator.get_param_vector() of a freshly built emulator:
log lambda_xi, log variance_c (c < m), log lengthscale_cp (component-major).  Row i of V is component i // M, grid point
i % M.  The Cholesky factor, its inverse and the solve are written with numpy vector operations so that they run in
longdouble (n <= 216: column loops are fast enough)."""
import numpy as np


def labels(m, P):
    return (["log_lambda_xi"] + [f"log_variance:{c}" for c in range(m)]
            + [f"log_lengthscale:{c}:{p}" for c in range(m) for p in range(P)])


def slot_derivatives(grid, iPhiPhi, row, dtype=np.float64):
    """V and [(label, dV / d label)] for every entry of `row`, in its order."""
    grid = np.asarray(grid, dtype=dtype)
    ipp = np.asarray(iPhiPhi, dtype=dtype)
    row = np.asarray(row, dtype=dtype)
    M, P = grid.shape
    n = ipp.shape[0]
    m = n // M
    assert n == m * M and row.shape == (1 + m + m * P,)
    lam = np.exp(row[0])
    var = np.exp(row[1:1 + m])
    ls = np.exp(row[1 + m:]).reshape(m, P)
    V = ipp / lam
    names = labels(m, P)
    D = [(names[0], -ipp / lam)]
    dvar, dls = [], []
    for c in range(m):
        sl = slice(c * M, (c + 1) * M)
        sq = ((grid[:, None, :] - grid[None, :, :]) / ls[c]) ** 2  # [g][h][p]
        K = var[c] * np.exp(-sq.sum(axis=-1) / 2)
        V[sl, sl] += K
        d = np.zeros((n, n), dtype=dtype)
        d[sl, sl] = K
        dvar.append(d)
        for p in range(P):
            d = np.zeros((n, n), dtype=dtype)
            d[sl, sl] = K * sq[:, :, p]
            dls.append(d)
    D += list(zip(names[1:1 + m], dvar)) + list(zip(names[1 + m:], dls))
    return V, D


def cholesky(A):
    L = np.zeros_like(A)
    for j in range(A.shape[0]):
        L[j, j] = np.sqrt(A[j, j] - L[j, :j] @ L[j, :j])
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def lower_inverse(L):
    X = np.zeros_like(L)
    for i in range(L.shape[0]):
        r = -(L[i, :i] @ X[:i])
        r[i] += 1
        X[i] = r / L[i, i]
    return X


def inverse_and_solve(V, w):
    """L, V^-1 = X^T X and alpha = V^-1 w."""
    L = cholesky(V)
    X = lower_inverse(L)
    G = X.T @ X
    return L, G, X.T @ (X @ np.asarray(w, dtype=V.dtype))


def log_likelihood(V, w):
    L = cholesky(V)
    z = lower_inverse(L) @ np.asarray(w, dtype=V.dtype)
    return -(2 * np.sum(np.log(np.diagonal(L))) + z @ z) / 2


def gradient(grid, iPhiPhi, w_hat, row, dtype=np.float64):
    """(lnL, the gradient in every entry of `row`) by the identity above."""
    V, D = slot_derivatives(grid, iPhiPhi, row, dtype)
    L, G, alpha = inverse_and_solve(V, w_hat)
    A = np.outer(alpha, alpha) - G
    lnl = -(2 * np.sum(np.log(np.diagonal(L))) + np.asarray(w_hat, dtype=dtype) @ alpha) / 2
    return lnl, np.array([np.sum(A * d) / 2 for _, d in D], dtype=dtype)
