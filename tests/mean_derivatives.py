"""Numpy restatement of the likelihood's gradient in the mean-flux parameters (vsini, vz, log_scale, Av, cheb:k and the
emulator's grid parameters), from the oracle's own pieces: rot_broaden's multiplier, quintic_knots / the collocation fit,
ccm89_a_lambda, cheb_correct's series, emulator_query's blocks and assemble_cov.  Test infrastructure only.

With r = flux - data, C the matrix that is factorised (jitter included), alpha = C^-1 r, X the scaled (m, N) emulator rows,
S = Sigma_w, V = C^-1 X^T, a = X alpha, za = S^-1 a, H = X V, G = S^-1 H S^-1, W = V S^-1:

    d lnL = - alpha^T df + sum_ki dX_ki (alpha_i za_k - W_ik) - 1/2 za^T dS za + 1/2 tr(dS G)

``tangents`` gives df, dX (transform parameters) or dmu, dS (grid parameters) per label in float64; ``gradient`` contracts
them in float64 or np.longdouble and returns, per label, the value and S_q: the same sum with every term replaced by its
absolute value."""
from math import factorial, pi

import numpy as np
from numpy.polynomial.chebyshev import chebval
from scipy.interpolate import BSpline
from scipy.special import j0, j1

from oracle import sf_oracle as O

LD = np.longdouble
SERIES_U = 2.0  # below: the power series of sb'; the closed form cancels like 20 eps / u^4


# --------------------------------------------------------------------------- d sb / d vsini
def _series_coefficient(k, dtype=LD):
    """c_k of sb(u) = sum_k (-1)^k c_k u^2k: 1 / (2^(2k+1) k! (k+1)!) + 3 (k+1) / (2k+3)!."""
    return dtype(1) / (dtype(2) ** (2 * k + 1) * factorial(k) * factorial(k + 1)) + dtype(3 * (k + 1)) / dtype(factorial(2 * k + 3))


def sb_prime_series(u, terms=40, dtype=LD):
    u = np.asarray(u, dtype=dtype)
    s = np.zeros_like(u)
    for k in range(terms, 0, -1):
        s = s * (u * u) + (-1) ** k * 2 * k * _series_coefficient(k, dtype)
    return s * u  # sum_k (-1)^k 2k c_k u^(2k-1)


def sb_prime_closed(u):
    u = np.asarray(u, dtype=np.float64)
    return j0(u) / u - 2 * j1(u) / u**2 + 3 * np.sin(u) / (2 * u**2) + 9 * np.cos(u) / (2 * u**3) - 9 * np.sin(u) / (2 * u**4)


def sb_prime(u):
    """sb'(u) in float64: the longdouble series below SERIES_U, the closed form above."""
    u = np.asarray(u, dtype=np.float64)
    small = u < SERIES_U
    out = np.empty_like(u)
    out[small] = sb_prime_series(u[small]).astype(np.float64)
    out[~small] = sb_prime_closed(u[~small])
    return out


def rot_multipliers(wave, n, vsini):
    """rot_broaden's multiplier per rfft bin and its derivative in vsini (bin 0: 1 and 0)."""
    dv = O.min_velocity_step(wave)
    u = (2.0 * pi * vsini * np.fft.rfftfreq(n, dv))[1:]
    sb = j1(u) / u - 3 * np.cos(u) / (2 * u**2) + 3.0 * np.sin(u) / (2 * u**3)
    return np.concatenate(([1.0], sb)), np.concatenate(([0.0], sb_prime(u) * u / vsini))


# --------------------------------------------------------------------------- the rows and their tangents
_FITS = {}


def _collocation_inverse(x):
    key = (len(x), float(x[0]), float(x[-1]))
    if key not in _FITS:
        ab, offs, t = O.quintic_collocation_band(x)
        A = np.zeros((len(x), len(x)))
        for i in range(len(x)):
            A[i, offs[i]: offs[i] + 6] = ab[i]
        _FITS[key] = (np.linalg.inv(A), t)
    return _FITS[key]


def cheb_series(order, p):
    return chebval(order.wave / order.wave.max(), [1, *p["cheb"]]) if "cheb" in p else np.ones(len(order.wave))


def row_tangents(order, p):
    """The m + 2 rows (eig_k, mean, std) on the data pixels behind broadening, Doppler shift, resampling, extinction and
    Chebyshev correction, and their derivatives in vsini, vz, Av and cheb:k (those the model has): (rows, {label: d rows})."""
    wave0 = order.min_dv_wave
    nf = len(wave0)
    spec = np.fft.rfft(order.bulk_fluxes)
    stack = [order.bulk_fluxes]
    if "vsini" in p:
        mult, dmult = rot_multipliers(wave0, nf, p["vsini"])
        stack = [np.fft.irfft(spec * mult, n=nf), np.fft.irfft(spec * dmult, n=nf)]
    Ainv, t = _collocation_inverse(wave0)
    s = np.sqrt((O.C_KMS + p["vz"]) / (O.C_KMS - p["vz"])) if "vz" in p else 1.0
    x = order.wave
    splines = [BSpline(t * s, Ainv @ y.T, 5, extrapolate=True) for y in stack]
    rows = splines[0](x).T
    ext = 10 ** (-0.4 * O.ccm89_a_lambda(x, p["Av"])) if "Av" in p else np.ones(len(x))
    pc = cheb_series(order, p)
    d = {}
    if "vsini" in p:
        d["vsini"] = splines[1](x).T * ext * pc
    if "vz" in p:
        d["vz"] = -splines[0].derivative()(x).T * x * O.C_KMS / (O.C_KMS**2 - p["vz"] ** 2) * ext * pc
    if "Av" in p:
        d["Av"] = -0.4 * np.log(10.0) * O.ccm89_a_lambda(x, 1.0) * (rows * ext * pc)
    for k in range(1, len(p.get("cheb", [])) + 1):
        d[f"cheb:{k}"] = rows * ext * chebval(x / x.max(), [0] * k + [1])
    return rows * ext * pc, d


def emulator_tangents(order, p):
    """mu, Sigma_w of emulator_query and their derivatives per grid parameter: (mu, S, [(dmu, dS), ...])."""
    g = order.grid_points
    theta = np.asarray(p["grid"], dtype=np.float64)
    m, M = order.m, len(g)
    v12 = O.rbf_blockdiag(g, theta[None, :], order.variances, order.lengthscales)  # (m M, m)
    sol = np.linalg.solve(order.v11, np.column_stack([order.w_hat, v12]))
    alpha, v11i_v12 = sol[:, 0], sol[:, 1:]
    mu = v12.T @ alpha
    S = np.diag(order.variances) - v12.T @ v11i_v12
    out = []
    for q in range(len(theta)):
        dv12 = np.zeros_like(v12)
        for i in range(m):
            dv12[i * M: (i + 1) * M, i] = v12[i * M: (i + 1) * M, i] * (g[:, q] - theta[q]) / order.lengthscales[i, q] ** 2
        cross = dv12.T @ v11i_v12
        out.append((dv12.T @ alpha, -(cross + cross.T)))
    return mu, S, out


def tangents(order, p, grid_names=("T", "logg", "Z")):
    """flux, X, Sigma_w as emulator_terms gives them (log_scale models) and per label the tangent: ("rows", df, dX) or
    ("grid", dmu, dS)."""
    rows, drows = row_tangents(order, p)
    mu, S, dgrid = emulator_tangents(order, p)
    sc = np.exp(p["log_scale"]) * p.get("norm", 1)
    eig, mean, std = rows[:-2], rows[-2], rows[-1]
    X = eig * std * sc
    flux = (mu @ (eig * std) + mean) * sc
    tan = {}
    for label, dr in drows.items():
        dX = (dr[:-2] * std + eig * dr[-1]) * sc
        tan[label] = ("rows", mu @ dX + dr[-2] * sc, dX)
    tan["log_scale"] = ("rows", flux, X)
    for name, (dmu, dS) in zip(grid_names, dgrid):
        tan[name] = ("grid", dmu, dS)
    return flux, X, S, tan


# --------------------------------------------------------------------------- the contraction
def cholesky(A):
    if A.dtype == np.float64:
        return np.linalg.cholesky(A)
    L = np.zeros_like(A)
    for j in range(A.shape[0]):
        L[j, j] = np.sqrt(A[j, j] - L[j, :j] @ L[j, :j])
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def solve_lower(L, B, transpose=False):
    """L^-1 B or L^-T B by substitution, in L's dtype."""
    n = L.shape[0]
    Y = np.array(B, dtype=L.dtype, copy=True)
    if not transpose:
        for i in range(n):
            Y[i] = (Y[i] - L[i, :i] @ Y[:i]) / L[i, i]
    else:
        for i in range(n - 1, -1, -1):
            Y[i] = (Y[i] - L[i + 1:, i] @ Y[i + 1:]) / L[i, i]
    return Y


def gradient(order, p, labels, dtype=np.float64, flux=None, pieces=None):
    """{label: (d lnL / d label, S_q)} with the contraction in ``dtype`` (the rows, tangents and the matrix are float64 values).
    flux: the model flux to take the residual from (default: the helper's own).  pieces: a dict that receives C, r, X, alpha, V,
    Sinv, za, W, G and tan (what an error bound is made of)."""
    f, X, S, tan = tangents(order, p)
    C = O.assemble_cov(order, p, X.copy(), S.copy())
    idx = np.arange(len(f))
    C[idx, idx] += O.JITTER
    r = ((f if flux is None else flux) - order.flux).astype(dtype)
    X, S = X.astype(dtype), S.astype(dtype)
    L = cholesky(C.astype(dtype))
    sol = solve_lower(L, solve_lower(L, np.column_stack([r, X.T])), transpose=True)
    alpha, V = sol[:, 0], sol[:, 1:]  # (N,), (N, m)
    Ls = cholesky(S)
    Sinv = solve_lower(Ls, solve_lower(Ls, np.eye(len(S), dtype=dtype)), transpose=True)
    a = X @ alpha
    za = Sinv @ a
    W = V @ Sinv
    G = Sinv @ (X @ V) @ Sinv
    if pieces is not None:
        pieces.update(C=C, r=r, X=X, alpha=alpha, V=V, Sinv=Sinv, a=a, za=za, W=W, G=G, tan=tan)
    out = {}
    for label in labels:
        kind, d0, d1 = tan[label]
        d0, d1 = d0.astype(dtype), d1.astype(dtype)
        if kind == "rows":
            t1, t2, t3 = -alpha * d0, d1.T * np.outer(alpha, za), -d1.T * W
        else:
            t1, t2, t3 = -d0 * a, -0.5 * np.outer(za, za) * d1, 0.5 * d1 * G
        out[label] = (t1.sum() + t2.sum() + t3.sum(), np.abs(t1).sum() + np.abs(t2).sum() + np.abs(t3).sum())
    return out
