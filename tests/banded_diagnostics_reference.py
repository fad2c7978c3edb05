"""The residual diagnostics on the band + Woodbury identity, restated in numpy for the tests (any dtype; the GPU tests use
np.longdouble).  With C = Bd + Y^T Y (Bd banded, Y: (m, n)) and right-hand sides R: (k, n), the sweep runs over the rows [R; Y]:

    T = Bd^-1 [R^T, Y^T]  (n, k + m),   G = [R; Y] T  ((k + m)^2, the Gram matrix),   S = I + G_YY = L_S L_S^T
    alpha_j = T_rj - T_Y S^-1 G_Y,rj          (column j of C^-1 R^T)
    Vs = T_Y L_S^-T (n, m),   C^-1 = Sigma - Vs Vs^T,  Sigma = Bd^-1
    diag(C^-1) = diag(Sigma) - rowsum(Vs^2)

and, pure host logic too, the term the alpha bound gains where the identity amplifies the solve's error."""
import numpy as np


def cholesky(A):
    """Lower Cholesky factor in the precision of A (numpy's LAPACK has no long double)."""
    A = np.asarray(A)
    L = np.zeros_like(A)
    for j in range(A.shape[0]):
        L[j, j] = np.sqrt(A[j, j] - L[j, :j] @ L[j, :j])
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def inverse_lower(L):
    """L^-1 by forward substitution, row by row, in the precision of L."""
    X = np.zeros_like(L)
    for i in range(L.shape[0]):
        row = -(L[i, :i] @ X[:i])
        row[i] += 1
        X[i] = row / L[i, i]
    return X


def sweep(Bd, Y, R):
    """T (n, k + m) and the Gram matrix G ((k + m)^2) of the rows [R; Y], with Sigma = Bd^-1, in the precision of Bd."""
    rows = np.vstack([np.atleast_2d(R), Y]).astype(Bd.dtype)
    Xl = inverse_lower(cholesky(Bd))
    Sigma = Xl.T @ Xl
    T = Sigma @ rows.T
    return dict(T=T, G=rows @ T, Sigma=Sigma, k=np.atleast_2d(R).shape[0])


def capacitance(G, k):
    """S = I + G_YY and its lower factor L_S."""
    m = G.shape[0] - k
    S = np.eye(m, dtype=G.dtype) + G[k:, k:]
    return S, cholesky(S)


def mix(T, G, k):
    """alpha (k, n): alpha_j = T_rj - T_Y S^-1 G_Y,rj from the sweep's T and Gram matrix."""
    _, Ls = capacitance(G, k)
    Li = inverse_lower(Ls)
    Z = Li.T @ (Li @ G[k:, :k])  # S^-1 G_Y,R
    return (T[:, :k] - T[:, k:] @ Z).T


def vs(T, G, k):
    """Vs = T_Y L_S^-T (n, m)."""
    _, Ls = capacitance(G, k)
    return T[:, k:] @ inverse_lower(Ls).T


def cinv_diag(sigma_diag, Vs):
    """diag(C^-1) = diag(Sigma) - rowsum(Vs^2), the sum over the columns ascending."""
    out = np.zeros_like(sigma_diag)
    for c in range(Vs.shape[1]):
        out = out + Vs[:, c] * Vs[:, c]
    return sigma_diag - out


def amplification(Bd, Y):
    """||Bd^-1||_inf ||Y^T Y||_inf: how much larger than C's own the residual of a solve through the identity may be.  The band
    solve leaves |Bd t - b| ~ u |Bd||t|, and t = Bd^-1 b is larger than alpha = C^-1 b by up to ||Bd^-1|| ||C||, so that
    C alpha - b inherits u ||Y^T Y|| ||Bd^-1|| ||b|| (Higham, Accuracy and Stability of Numerical Algorithms, section 26 on the
    Sherman-Morrison-Woodbury formula: it is not backward stable when Bd is much worse conditioned than the update)."""
    Sigma = np.linalg.inv(np.asarray(Bd, dtype=np.float64))
    Y = np.asarray(Y, dtype=np.float64)
    return float(np.abs(Sigma).sum(axis=1).max() * np.abs(Y.T @ Y).sum(axis=1).max())
