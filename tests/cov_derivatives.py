"""The two structured covariance kernels and their derivatives in the hyper-parameters, in numpy, in the dtype of the
wavelengths (np.longdouble in gives np.longdouble out).  A helper of the gradient tests, not a test.

Global kernel (kernels.py:27-40), u = r / ls, t = 1/2 + 1/2 cos(pi u / 6), g = (1 + sqrt(3) u) exp(-sqrt(3) u):
    K = A t g,   dK/dlog_amp = K,   dK/dlog_ls = -u A (t' g + t g'),   t' = -(pi / 12) sin(pi u / 6),  g' = -3 u exp(-sqrt(3) u)
Local kernel (kernels.py:69-80), d(w) = c / mu |w - mu|, d' = -c sign(w - mu) w / mu^2, v = r_tap / sigma,
e = exp(-r2 / (2 sigma^2)), t = 1/2 + 1/2 cos(pi v / 4), s = 1/2 sin(pi v / 4), r_tap' = d' of the larger metric (the column's
on a tie):
    K = A t e,   dK/dlog_amp = K,   dK/dlog_sigma = A e (s pi v / 4 + t r2 / sigma^2),
    dK/dmu = A e (-s pi / (4 sigma) r_tap' - t (d_col d_col' + d_row d_row') / sigma^2)
Everything is 0 outside the cut-off (r <= 6 ls, r_tap <= 4 sigma).  ``absolute=True`` gives the same sums with the absolute
value taken term by term: the size a rounding-error bound of the derivative entry has to be measured against."""
import numpy as np

C_KMS = 2.99792458e5
GLOBAL_SLOTS = ("log_amp", "log_ls")
LOCAL_SLOTS = ("mu", "log_amp", "log_sigma")


def _typed(wave, *values):
    w = np.asarray(wave)
    if w.dtype not in (np.float64, np.longdouble):
        w = w.astype(np.float64)
    T = w.dtype.type
    return (w, T) + tuple(T(v) for v in values)


def global_kernel(wave, log_amp, log_ls, absolute=False):
    """dict K, log_amp, log_ls of (n, n) arrays: row = wave[:, None], column = wave[None, :]."""
    w, T, log_amp, log_ls = _typed(wave, log_amp, log_ls)
    amp, ls = np.exp(log_amp), np.exp(log_ls)
    wi, wj = w[None, :], w[:, None]
    r = T(C_KMS) / 2 * np.abs((wi - wj) / (wi + wj))
    r0 = 6 * ls
    inside = r <= r0
    rr = np.where(inside, r, T(0))
    s3 = np.sqrt(T(3))
    taper = T(0.5) + T(0.5) * np.cos(np.pi * rr / r0)
    K = np.where(inside, taper * amp * (1 + s3 * rr / ls) * np.exp(-s3 * rr / ls), T(0))  # the oracle's order of operations
    u = rr / ls
    tp = -(np.pi / 12) * np.sin(np.pi * u / 6)
    e = np.exp(-s3 * u)
    g, gp = (1 + s3 * u) * e, -3 * u * e
    if absolute:
        d_ls = u * amp * (np.abs(tp) * g + taper * np.abs(gp))
    else:
        d_ls = -u * amp * (tp * g + taper * gp)
    return dict(K=K, log_amp=K, log_ls=np.where(inside, d_ls, T(0)))


def local_kernel(wave, mu, log_amp, log_sigma, absolute=False):
    """dict K, mu, log_amp, log_sigma of (n, n) arrays."""
    w, T, mu, log_amp, log_sigma = _typed(wave, mu, log_amp, log_sigma)
    amp, sigma = np.exp(log_amp), np.exp(log_sigma)
    d = T(C_KMS) / mu * np.abs(w - mu)
    dp = -T(C_KMS) * np.sign(w - mu) * w / (mu * mu)
    di, dj = d[None, :], d[:, None]  # column, row
    dpi, dpj = dp[None, :], dp[:, None]
    col = di >= dj
    r_tap = np.where(col, di, dj)
    r_tap_p = np.where(col, dpi, dpj)
    r2 = di**2 + dj**2
    r0 = 4 * sigma
    inside = r_tap <= r0
    rt = np.where(inside, r_tap, T(0))
    r2i = np.where(inside, r2, T(0))
    taper = T(0.5) + T(0.5) * np.cos(np.pi * rt / r0)
    K = np.where(inside, taper * amp * np.exp(-T(0.5) * r2i / sigma**2), T(0))  # the oracle's order of operations
    v = rt / sigma
    s = T(0.5) * np.sin(np.pi * v / 4)
    ae = amp * np.exp(-T(0.5) * r2i / sigma**2)
    if absolute:
        d_sig = ae * (np.abs(s) * np.pi * v / 4 + taper * r2i / sigma**2)
        d_mu = ae * (np.abs(s) * np.pi / (4 * sigma) * np.abs(r_tap_p) + taper * (np.abs(di * dpi) + np.abs(dj * dpj)) / sigma**2)
    else:
        d_sig = ae * (s * np.pi * v / 4 + taper * r2i / sigma**2)
        d_mu = ae * (-s * np.pi / (4 * sigma) * r_tap_p - taper * (di * dpi + dj * dpj) / sigma**2)
    zero = T(0)
    return dict(K=K, mu=np.where(inside, d_mu, zero), log_amp=K, log_sigma=np.where(inside, d_sig, zero))


def slot_derivatives(wave, p, absolute=False, dtype=np.float64):
    """The derivative matrices of an oracle parameter dict ``p`` in the device's slot order: log_amp, log_ls of the global
    kernel if present, then mu, log_amp, log_sigma per local kernel.  List of (name, (n, n) array)."""
    w = np.asarray(wave).astype(dtype)
    out = []
    if "global_cov" in p:
        g = global_kernel(w, *p["global_cov"], absolute=absolute)
        out += [("global_cov:" + s, g[s]) for s in GLOBAL_SLOTS]
    for k, (mu, la, ls) in enumerate(p.get("local_cov", [])):
        l = local_kernel(w, mu, la, ls, absolute=absolute)
        out += [(f"local_cov:{k}:{s}", l[s]) for s in LOCAL_SLOTS]
    return out
