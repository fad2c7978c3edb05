"""The Fisher information of the mean-flux parameters at fixed covariance, F = J^T C^-1 J with J = [d f / d theta_j], restated
in numpy from the tangents of tests/mean_derivatives.py and the oracle's matrix, and the reference-only bound its entries are
held to.  Test infrastructure only.

    dense      C = L L^T (jitter included),  Z = L^-1 J,  F = Z^T Z
    Woodbury   C = Bd + Y^T Y,  G = R^T Bd^-1 R for the rows R = [Y; J],  S = I + G_YY = L_S L_S^T,  U = L_S^-1 G_YJ,
               F = G_JJ - U^T U

The bound on entry (i, j), from the np.longdouble dense F alone (``entry_bound``), is the sum of
  1. the solve: solve_factor(N) sqrt(F_ii F_jj)  (the backward error of a Cholesky solve, tests/banded_derivatives.py, on both
     factors of the bilinear form, Cauchy-Schwarz in the C^-1 inner product);
  2. the transform contract, 1e-10 max|column| on every entry of a tangent column, to first order through both factors:
     |dJ_i|^T |C^-1 J_j| + |C^-1 J_i|^T |dJ_j| = 1e-10 (max|J_i| |C^-1 J_j|_1 + max|J_j| |C^-1 J_i|_1);
  3. the sum itself: gamma_N sum_l |Z_li| |Z_lj|;
  4. for the band solver, the same factor as 1. on sqrt(G_JJ,ii G_JJ,jj): F is the difference G_JJ - U^T U;
  5. what is not derived (another order of summation, the rounding of the rows): 8 |F_float64 - F_longdouble|."""
import numpy as np

import banded_derivatives as BD
import mean_derivatives as MD
from oracle import sf_oracle as O

LD = np.longdouble


def jacobian(order, p, labels):
    """(J (N, len(labels)), X, Sigma_w): a "rows" tangent takes its d f, a "grid" tangent d mu^T X."""
    f, X, S, tan = MD.tangents(order, p)
    cols = []
    for label in labels:
        kind, d0, _ = tan[label]
        cols.append(d0 if kind == "rows" else d0 @ X)
    return np.column_stack(cols), X, S


def covariance(order, p, X, S, jitter=True):
    C = O.assemble_cov(order, p, X.copy(), S.copy())
    if jitter:
        idx = np.arange(C.shape[0])
        C[idx, idx] += O.JITTER
    return C


def whitened(J, C, dtype=np.float64):
    """Z = L^-1 J in ``dtype``."""
    return MD.solve_lower(MD.cholesky(C.astype(dtype)), J.astype(dtype))


def fisher_dense(J, C, dtype=np.float64):
    Z = whitened(J, C, dtype)
    return Z.T @ Z


def fisher_woodbury(J, Bd, Y, dtype=np.float64, drop_uu=False):
    """(F, G_JJ) by the band solve and the capacitance step; ``drop_uu``: a wrong-weight variant for the tests (U^T U omitted)."""
    m = Y.shape[0]
    R = np.column_stack([Y.T.astype(dtype), J.astype(dtype)])
    G = R.T @ BD.band_solve(Bd, R, dtype)
    Ls = MD.cholesky(np.eye(m, dtype=dtype) + G[:m, :m])
    U = MD.solve_lower(Ls, G[:m, m:])
    GJJ = G[m:, m:]
    return (GJJ if drop_uu else GJJ - U.T @ U), GJJ


def reference(order, p, labels):
    """Everything the checks of one walker need, made once: J, C, the pieces of the Woodbury form, F in float64 and longdouble
    (dense), G_JJ and the terms of the bound."""
    J, X, S = jacobian(order, p, labels)
    C = covariance(order, p, X, S)
    q = BD.pieces(order, p)
    Zld = whitened(J, C, LD)
    Fld = Zld.T @ Zld
    F64 = fisher_dense(J, C)
    Fw, GJJ = fisher_woodbury(J, q["Bd"], q["Y"])
    L = MD.cholesky(C.astype(LD))
    CiJ = np.abs(MD.solve_lower(L, Zld, transpose=True)).astype(np.float64)  # |C^-1 J|
    return dict(J=J, C=C, Bd=q["Bd"], Y=q["Y"], Fld=Fld, F64=F64, Fw=Fw, GJJ=GJJ, Zabs=np.abs(Zld).astype(np.float64), CiJ=CiJ,
                labels=tuple(labels))


def entry_bound(ref, banded=False):
    """The (p, p) bound of the module docstring and its terms (dict), from ``reference``'s result."""
    N = ref["J"].shape[0]
    F = ref["Fld"].astype(np.float64)
    d = np.sqrt(np.diag(F))
    fac = BD.solve_factor(N)
    solve = fac * np.outer(d, d)
    jmax, l1 = np.abs(ref["J"]).max(axis=0), ref["CiJ"].sum(axis=0)
    contract = 1e-10 * (np.outer(jmax, l1) + np.outer(l1, jmax))
    sums = BD.gamma(N) * (ref["Zabs"].T @ ref["Zabs"])
    g = np.sqrt(np.diag(ref["GJJ"]))
    band = fac * np.outer(g, g) if banded else np.zeros_like(F)
    other = 8 * np.abs(ref["F64"] - F)
    terms = dict(solve=solve, contract=contract, sums=sums, band=band, other=other)
    return solve + contract + sums + band + other, terms


def normalised(F):
    d = np.sqrt(np.diag(F).astype(np.float64))
    return np.asarray(F, dtype=np.float64) / np.outer(d, d)
