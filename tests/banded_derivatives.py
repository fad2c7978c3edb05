"""The mean gradient's solve on the band + Woodbury identity, restated for the tests, and the reference-only bound the mean
gradient's slots are held to (the one of tests/test_gpu_mean_gradient.py, items 1 - 4 of its docstring, as a function).

    C = Bd + Y^T Y,  Y = Lw^-1 X,  Sigma_w = Lw Lw^T        (the oracle's C = X^T Sigma_w^-1 X + sigma^2 + K + jitter)
    T = Bd^-1 [r, Y^T],  gram = [r, Y^T]^T T = [[g_rr, g^T], [g, G_YY]],  S = I + G_YY
    alpha = t_r - T_Y S^-1 g,   V = C^-1 X^T = T_Y S^-1 Lw^T,   so  [alpha, V] = T M

float64: scipy's cholesky_banded + cho_solve_banded on the lower band storage of Bd; np.longdouble: the dense substitutions of
tests/mean_derivatives.py on Bd."""
import numpy as np
from scipy.linalg import cho_solve_banded, cholesky_banded, solve_triangular

import mean_derivatives as MD
from oracle import sf_oracle as O

U = 2.0 ** -53
LD = np.longdouble


def gamma(k):
    return k * U / (1 - k * U)


def solve_factor(N):
    """fac of the residual bound |A x - b|_inf <= fac (|A|_inf |x|_inf + |b|_inf) (tests/test_gpu_apply_factor.py)."""
    return 1e-13 + N * gamma(3 * N + 1)


def pieces(order, p, flux=None):
    """Bd (dense, jitter included), Y, Lw, X, r and C of the oracle's model: what the band call factorises and solves for."""
    f, X, S, _ = MD.tangents(order, p)
    idx = np.arange(len(f))
    Bd = O.assemble_cov(order, p, np.zeros_like(X), S.copy())
    C = O.assemble_cov(order, p, X.copy(), S.copy())
    Bd[idx, idx] += O.JITTER
    C[idx, idx] += O.JITTER
    Lw = np.linalg.cholesky(S)
    Y = solve_triangular(Lw, X, lower=True)
    r = (f if flux is None else flux) - order.flux
    return dict(Bd=Bd, Y=Y, Lw=Lw, X=X, r=r, C=C, S=S)


def halfwidth(Bd):
    i, j = np.nonzero(Bd)
    return int(np.abs(i - j).max())


def lower_band(A, w):
    """scipy's lower band storage: ab[d, j] = A[j + d, j]."""
    n = A.shape[0]
    ab = np.zeros((w + 1, n))
    for d in range(w + 1):
        ab[d, : n - d] = A[np.arange(d, n), np.arange(n - d)]
    return ab


def band_solve(Bd, rhs, dtype=np.float64):
    """Bd^-1 rhs (rhs: (N, k))."""
    if dtype == np.float64:
        return cho_solve_banded((cholesky_banded(lower_band(Bd, halfwidth(Bd)), lower=True), True), rhs)
    L = MD.cholesky(Bd.astype(dtype))
    return MD.solve_lower(L, MD.solve_lower(L, rhs.astype(dtype)), transpose=True)


def mix_matrix(gram, Lw):
    """M ((1 + m) x (1 + m)) with [alpha, V] = T M, in gram's dtype."""
    dtype = gram.dtype
    m = gram.shape[0] - 1
    Ls = MD.cholesky(np.eye(m, dtype=dtype) + gram[1:, 1:])
    Z = MD.solve_lower(Ls, MD.solve_lower(Ls, np.column_stack([gram[1:, 0], Lw.T.astype(dtype)])), transpose=True)
    M = np.zeros((1 + m, 1 + m), dtype=dtype)
    M[0, 0] = 1
    M[1:, 0] = -Z[:, 0]
    M[1:, 1:] = Z[:, 1:]
    return M


def alpha_V(q, dtype=np.float64):
    """(alpha (N,), V (N, m)) of pieces() through the band solve and the mix.  In another dtype than float64 Lw and Y are formed
    in it from the float64 Sigma_w and X."""
    Lw, Y = q["Lw"], q["Y"]
    if dtype != np.float64:
        Lw = MD.cholesky(q["S"].astype(dtype))
        Y = MD.solve_lower(Lw, q["X"].astype(dtype))
    rhs = np.column_stack([q["r"].astype(dtype), Y.T])
    T = band_solve(q["Bd"], rhs, dtype)
    sol = T @ mix_matrix(rhs.T @ T, Lw)
    return sol[:, 0], sol[:, 1:]


def check_slots(name, oo, plist, labels, out, hard=True):
    """Every slot of out["grad"] against the np.longdouble contraction of tests/mean_derivatives.py: the bound of
    tests/test_gpu_mean_gradient.py (solve, transform contract, sums, another order of summation) and the wrong-weight guard
    1e-6 S_q against the float64 helper.  Prints every figure; asserts both when ``hard``.  Returns the largest err / bound."""
    N = len(oo.wave)
    worst = 0.0
    fac = solve_factor(N)
    for b, p in enumerate(plist):
        flux = out["flux"][b]
        ref64 = MD.gradient(oo, p, labels)
        q = {}
        refld = MD.gradient(oo, p, labels, dtype=LD, flux=flux, pieces=q)
        own64 = MD.gradient(oo, p, labels, flux=flux)
        m = q["X"].shape[0]
        ab = lambda v: np.abs(v).astype(np.float64)  # noqa: E731
        aCi, aX, aSi, aal, aza = np.abs(np.linalg.inv(q["C"])), ab(q["X"]), ab(q["Sinv"]), ab(q["alpha"]), ab(q["za"])
        cnorm, rowsum = np.abs(q["C"]).sum(axis=1).max(), aCi.sum(axis=1)
        d_alpha = rowsum * fac * (cnorm * aal.max() + ab(q["r"]).max())
        d_V = np.stack([rowsum * fac * (cnorm * ab(q["V"][:, k]).max() + aX[k].max()) for k in range(m)], axis=1)
        omega = np.outer(aal, aza) + ab(q["W"])  # (N, m)
        for j, label in enumerate(labels):
            got = out["grad"][b, j]
            kind, d0, d1 = q["tan"][label]
            d0, d1 = np.abs(d0), np.abs(d1)
            sq = float(refld[label][1])
            if kind == "rows":
                solve = (d_alpha @ (d0 + d1.T @ aza) + np.sum(d1.T * np.outer(aal, aSi @ (aX @ d_alpha)))
                         + np.sum(d1.T * (d_V @ aSi)))
                contract = 1e-10 * (d0.max() * aal.sum() + d1.max() * omega.sum())
                k = N * (1 + 2 * m)
            else:
                da = aX @ d_alpha
                solve = d0 @ da + aza @ (d1 @ (aSi @ da)) + 0.5 * np.sum(d1 * (aSi @ (aX @ d_V) @ aSi))
                contract = 0.0
                k = m + 2 * m * m
            other_order = 8 * abs(float(own64[label][0] - refld[label][0]))
            bound = solve + contract + (gamma(k) + 3 * U) * sq + other_order + 1e-10 * sq
            err = abs(float(got - refld[label][0]))
            guard = abs(got - ref64[label][0]) / float(ref64[label][1])
            worst = max(worst, err / bound)
            print(f"{name} walker {b} {label}: {got!r}, err / bound = {err / bound:.3g} (bound {bound:.3g}: solve {solve:.3g}, "
                  f"contract {contract:.3g}, 8 x |float64 - longdouble| {other_order:.3g}), S_q {sq:.3g}, "
                  f"|got - float64 helper| / S_q = {guard:.3g}")
            if hard:
                assert guard <= 1e-6, (name, b, label, got, ref64[label])
                assert err <= bound, (name, b, label, got, float(refld[label][0]), err, bound)
    print(f"{name}: largest err / bound = {worst:.3g}")
    return worst
