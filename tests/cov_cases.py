"""Cases and CPU references for the covariance-structure tests (tests/test_gpu_cov_structure.py,
tests/test_cov_reference.py): wavelength grids that leave the log-uniform corner of the walker ball, per-walker
structure that reaches tiles only through their corners, 128-pixel tile boundaries, the array edges and the limits of
the library, and three references built from the oracle's pieces:

* ``dense_cov``       the oracle's dense covariance (``dense_loglike``: its likelihood).  The structured kernels are
                      evaluated with the oracle's element functions on the rows / columns their support reaches only
                      and added to an explicit zero elsewhere: the same bits as ``O.forward_model`` (``test_cov_reference.py`` pins
                      that) without 32 dense N x N evaluations per walker;
* ``band_woodbury``   the same likelihood from a band matrix (sigma^2 + structured kernels + jitter, LAPACK band
                      Cholesky) and a Woodbury step for the rank-m emulator term -- usable at N where no dense matrix
                      fits the host;
* ``farthest_block``  the sensitivity probe: the structured entries of the farthest-off-diagonal 128 x 128 block,
                      whose removal a case must be able to detect."""
import numpy as np
from scipy.linalg import cho_factor, cho_solve, cho_solve_banded, cholesky_banded

from oracle import sf_oracle as O
from starfish_amd import synth

TILE = 128
LOGDET_RTOL = 1e-10  # tolerances of the repository's likelihood parity tests
SQMAH_RTOL = 1e-8
LOGUNIFORM_SPREAD = 2e-10  # the library's log-uniform test (sf_ctx_create): (qmax - qmin) <= 2e-10 qmax


def q_spread(wave):
    """Relative spread of (w_i - w_{i-1}) / (w_i + w_{i-1}): the library's log-uniform detection, restated."""
    w = np.asarray(wave, dtype=np.float64)
    q = (w[1:] - w[:-1]) / (w[1:] + w[:-1])
    return (q.max() - q.min()) / q.max()


# ------------------------------------------------------------------------------------------------ grids
GRIDS = ("G1", "G2", "G3", "G4", "G5")


def make_grid_order(kind, N, m=8, seed=0):
    """One synthetic order of N pixels on grid ``kind``:
    G1 log-uniform (the K_global table path), G2 pixel spacing modulated by 5 % (per-entry path), G3 log-uniform with
    three gaps of 4, 60 and 200 pixels cut out and a smoothly varying per-pixel sigma in [0.005, 0.03], G4 two sorted
    segments where the second starts below the end of the first (culling off), G5 log-uniform only to within the
    library's detection threshold (relative spread of the pixel ratio ~1.5e-10)."""
    rng = np.random.default_rng(1000 + seed)
    if kind == "G3":
        o = synth.make_order(N=N + 264, m=m, seed=seed)
        keep = np.ones(N + 264, dtype=bool)
        for start, width in ((N // 5, 4), (N // 2, 60), ((4 * N) // 5, 200)):
            keep[start : start + width] = False
        o = dict(o)
        o["wave"] = o["wave"][keep]
    else:
        o = dict(synth.make_order(N=N, m=m, seed=seed))
    w = o["wave"]
    if kind == "G2":
        o = synth.perturb_grid(o)
        w = o["wave"]
    elif kind == "G4":
        h = N // 2
        step = np.log(w[1] / w[0])
        w = np.concatenate([w[:h], w[h:] * np.exp(-40.5 * step)])
        assert w[h] < w[h - 1] and np.all(np.diff(w[:h]) > 0) and np.all(np.diff(w[h:]) > 0)
    elif kind == "G5":
        step = np.log(w[1] / w[0])
        i = np.arange(N - 1)
        for amp in (0.7e-10, 0.6e-10, 0.5e-10, 0.4e-10, 0.3e-10):  # (the rounding of the grid adds its own spread)
            w = w[0] * np.exp(np.concatenate([[0.0], np.cumsum(step * (1 + amp * np.sin(i / 50.0 + 0.3)))]))
            if q_spread(w) <= 0.8 * LOGUNIFORM_SPREAD:
                break
        spread = q_spread(w)
        assert 1e-10 <= spread <= 0.8 * LOGUNIFORM_SPREAD, spread  # still the table path, but not to rounding
    o["wave"] = w
    o["flux"] = 1 + 0.1 * np.sin(w / 7) + 0.01 * rng.standard_normal(len(w))
    if kind == "G3":
        # smooth random sigma in [0.005, 0.03]: a diagonal read at a shifted index is not invisible
        x = np.linspace(0, 1, len(w))
        s = sum(rng.standard_normal() * np.sin(2 * np.pi * (k + 1) * x + rng.uniform(0, 6)) for k in range(6))
        s = (s - s.min()) / (s.max() - s.min())
        o["sigma"] = 0.005 + 0.025 * s
    else:
        o["sigma"] = 0.01 * np.ones(len(w))
    return o


def oracle_order_of(o):
    """OracleOrder of a synthetic order.  The emulator's resampling grid comes from the sorted wavelengths (an unsorted
    grid has no meaningful minimum velocity step: the reference's log-lambda grid needs one)."""
    w = o["wave"]
    base = dict(o)
    base["wave"] = np.sort(w)
    oo = O.OracleOrder(base["wave"], o["flux"], o["sigma"], o["emu_wl"], o["eigenspectra"], o["flux_mean"],
                       o["flux_std"], o["grid_points"], o["w_hat"])
    oo.wave = np.asarray(w, dtype=np.float64)
    return oo


# ------------------------------------------------------------------------------------------------ structure
def pixel_metric(wave):
    """Median metric step of the global kernel between neighbouring pixels, c/2 |dw| / (w_i + w_j) (km/s)."""
    w = np.asarray(wave)
    return float(np.median(np.abs(O.C_KMS / 2 * (w[1:] - w[:-1]) / (w[1:] + w[:-1]))))


def global_reaching(wave, pixels, log_amp):
    """Global kernel whose support radius 6 ls is ``pixels`` pixels."""
    return (log_amp, float(np.log(pixels * pixel_metric(wave) / 6)))


def many_locals(wave, n, variant=0):
    """n <= 32 local kernels (mu, log_amp, log_sigma): at both array edges, 0.3 A outside the range on both sides, on
    128-pixel tile boundaries of the matrix's own frame and of the frame shifted by 64, an overlapping pair, one whose
    patch spans ~300 pixels, one narrower than a pixel; the rest spread along the order.  ``variant`` moves the
    boundary kernels by one pixel and the spread ones by a third of their spacing (different tile maps per walker)."""
    w = np.asarray(wave)
    N = len(w)
    ls = np.log
    s = variant
    edge = [
        (w[0], -7.0, ls(15.0)), (w[-1], -7.0, ls(15.0)),
        (w[0] - 0.3, -6.5, ls(30.0)), (w[-1] + 0.3, -6.5, ls(30.0)),
    ]
    bound = [(w[i + s], -7.5, ls(5.0)) for i in (127, 128, 255, 256, 63, 64, 191, 192)]
    special = [
        (w[N // 2], -7.0, ls(20.0)), (w[N // 2 + 10], -7.0, ls(20.0)),  # overlapping pair
        # 2 x 4 sigma = 600 km/s, ~300 px at dv = 2, centred 64 px into a tile: its farthest 128 x 128 block (two tiles off
        # the diagonal) holds entries half a patch from mu, not only the vanishing corners of the patch
        (w[TILE * (N // (3 * TILE) + s) + 64], -6.0, ls(75.0)),
        (w[(2 * N) // 3], -6.0, ls(0.2)),                                  # narrower than a pixel
    ]
    out = (edge + bound + special)[:n]
    rest = n - len(out)
    for k in range(rest):
        i = int(N * (0.05 + 0.9 * (k + (s % 3) / 3.0) / max(rest, 1)))
        out.append((w[min(i, N - 1)], -8.0 + 0.1 * (k % 5), ls(8.0 + k % 7)))
    return [(float(a), float(b), float(c)) for a, b, c in out]


def base_params(k):
    """Stellar / calibration part of walker k (structure comes separately)."""
    return dict(vz=10.0 + 0.3 * k, vsini=30.0 - 0.5 * k, log_scale=0.01 * k, cheb=[0.01, -0.02 + 0.002 * k],
                grid=[6050.0 + 20 * k, 4.2 + 0.03 * k, -0.3 - 0.02 * k])


def batch(o, kind, n_local=32):
    """Three walkers of one model structure (``kind``), each with a different tile map:
    'A' global + n_local locals (band reaching 128 + 64 px, 256 + 64 px, narrower than a pixel),
    'G' global only (the same three bands), 'L' n_local locals only, 'N' no structured kernel."""
    w = o["wave"]
    bands = [global_reaching(w, 128 + 64, -5.5), global_reaching(w, 2 * 128 + 64, -3.5),
             (-6.0, float(np.log(0.4 * pixel_metric(w) / 6)))]
    out = []
    for k in range(3):
        p = base_params(k)
        if kind in ("A", "G"):
            p["global_cov"] = bands[k]
        if kind in ("A", "L"):
            p["local_cov"] = many_locals(w, n_local, variant=k)
        out.append(p)
    return out


# ------------------------------------------------------------------------------------------------ references
def structured_part(oo, p):
    """K_global + sum K_local of the oracle (dense, zero outside the supports), element functions of the oracle in
    its order of additions; the local kernels are evaluated on the pixels their patch reaches only."""
    w = oo.wave
    n = len(w)
    S = np.zeros((n, n))
    if "global_cov" in p:
        la, ll = p["global_cov"]
        S += O.matern32_global(w, np.exp(la), np.exp(ll))
    if p.get("local_cov"):
        loc = np.zeros((n, n))
        for mu, la, ls in p["local_cov"]:
            d = O.local_metric(w, mu)
            sig = np.exp(ls)
            idx = np.nonzero(d <= 4 * sig)[0]
            if idx.size:
                ds = d[idx]
                loc[np.ix_(idx, idx)] += O.gaussian_local_elem(ds[None, :], ds[:, None], np.exp(la), sig)
        S += loc
    return S


def dense_cov(oo, p):
    """O.forward_model's (flux, cov, scale) with the structured part from ``structured_part``."""
    flux, X, w_cov, scale = O.emulator_terms(oo, p)
    fac = cho_factor(w_cov)
    cov = X.T @ cho_solve(fac, X)
    idx = np.arange(len(oo.wave))
    cov[idx, idx] += oo.sigma**2
    if "global_cov" in p:
        la, ll = p["global_cov"]
        cov += O.matern32_global(oo.wave, np.exp(la), np.exp(ll))
    if p.get("local_cov"):
        cov += structured_part(oo, dict(local_cov=p["local_cov"]))
    return flux, cov, scale


def dense_loglike(oo, flux, cov):
    """O.log_likelihood on a given covariance: (lnl, logdet, sqmah)."""
    c = cov.copy()
    idx = np.arange(len(flux))
    c[idx, idx] += O.JITTER
    fac = cho_factor(c, overwrite_a=True)
    logdet = 2 * np.sum(np.log(fac[0].diagonal()))
    R = flux - oo.flux
    sqmah = R @ cho_solve(fac, R)
    return -(logdet + sqmah) / 2, logdet, sqmah


def farthest_block(S):
    """(I, J) of the 128 x 128 block with the largest I - J (lower triangle) that holds a non-zero entry of the
    structured part S, or None when S is zero."""
    n = S.shape[0]
    nb = (n + TILE - 1) // TILE
    best = None
    for I in range(nb):
        for J in range(I + 1):
            if best is not None and I - J <= best[0] - best[1]:
                continue
            if np.any(S[I * TILE : (I + 1) * TILE, J * TILE : (J + 1) * TILE]):
                best = (I, J)
    return best


def drop_block_logdet(cov, S, blk):
    """logdet of cov + jitter with the structured part of block blk (and of its mirror) removed."""
    I, J = blk
    c = cov.copy()
    rs, cs = slice(I * TILE, (I + 1) * TILE), slice(J * TILE, (J + 1) * TILE)
    c[rs, cs] -= S[rs, cs]
    if I != J:
        c[cs, rs] -= S[cs, rs]
    idx = np.arange(c.shape[0])
    c[idx, idx] += O.JITTER
    try:
        L = cho_factor(c, overwrite_a=True)[0]
    except np.linalg.LinAlgError:
        return np.inf  # not even positive definite without the block: a dropped tile could not go unnoticed
    return 2 * np.sum(np.log(L.diagonal()))


def band_woodbury(oo, p, hw, drop_rows_from=None):
    """-(logdet + sqmah) / 2 of C = B + X^T W^-1 X without forming C: B = diag(sigma^2) + K_global + sum K_local + jitter
    held as a band of half-width hw (LAPACK dpbtrf), W = w_cov, logdet C = logdet B + logdet(W + X B^-1 X^T) - logdet W,
    R^T C^-1 R = R^T B^-1 R - (X B^-1 R)^T (W + X B^-1 X^T)^-1 (X B^-1 R).  Needs a sorted grid; asserts that the
    structure's support fits the band.  ``drop_rows_from``: leave out the structured entries of every row and column
    from that index on (sensitivity probe).  Returns (lnl, logdet, sqmah)."""
    w = oo.wave
    n = len(w)
    assert np.all(np.diff(w) > 0), "the band reference needs a sorted grid"
    ab = np.zeros((hw + 1, n))  # ab[d, j] = B[j + d, j]
    if "global_cov" in p:
        la, ll = p["global_cov"]
        amp, lsc = np.exp(la), np.exp(ll)
        for d in range(hw + 1):
            ab[d, : n - d] += O.matern32_elem(w[: n - d], w[d:], amp, lsc)
        if hw + 1 < n:
            assert not np.any(O.matern32_elem(w[: n - hw - 1], w[hw + 1 :], amp, lsc)), "global kernel wider than the band"
    if p.get("local_cov"):
        loc = np.zeros_like(ab)
        for mu, la, ls in p["local_cov"]:
            d_ = O.local_metric(w, mu)
            sig = np.exp(ls)
            idx = np.nonzero(d_ <= 4 * sig)[0]
            if not idx.size:
                continue
            assert idx[-1] - idx[0] <= hw, "local kernel wider than the band"
            for d in range(min(hw, idx[-1] - idx[0]) + 1):
                loc[d, : n - d] += O.gaussian_local_elem(d_[: n - d], d_[d:], np.exp(la), sig)
        ab += loc
    if drop_rows_from is not None:
        for d in range(hw + 1):
            # entry (j + d, j) reaches the dropped rows / columns when j + d >= drop_rows_from
            ab[d, max(drop_rows_from - d, 0) :] = 0.0
    ab[0] += oo.sigma**2
    ab[0] += O.JITTER
    flux, X, w_cov, _ = O.emulator_terms(oo, p)
    cb = cholesky_banded(ab, lower=True)
    logdet_b = 2 * np.sum(np.log(cb[0]))
    R = flux - oo.flux
    BiR = cho_solve_banded((cb, True), R)
    BiXt = cho_solve_banded((cb, True), X.T)
    S = w_cov + X @ BiXt
    fs = cho_factor(S)
    fw = cho_factor(w_cov)
    logdet = logdet_b + 2 * np.sum(np.log(np.diag(fs[0]))) - 2 * np.sum(np.log(np.diag(fw[0])))
    u = X @ BiR
    sqmah = R @ BiR - u @ cho_solve(fs, u)
    return -(logdet + sqmah) / 2, logdet, sqmah


def support_halfwidth(oo, p):
    """Smallest band half-width that holds the structure of p on a sorted grid."""
    w = oo.wave
    n = len(w)
    hw = 0
    if "global_cov" in p:
        la, ll = p["global_cov"]
        amp, lsc = np.exp(la), np.exp(ll)
        while hw + 1 < n and np.any(O.matern32_elem(w[: n - hw - 1], w[hw + 1 :], amp, lsc)):
            hw += 1
    for mu, la, ls in p.get("local_cov", []):
        idx = np.nonzero(O.local_metric(w, mu) <= 4 * np.exp(ls))[0]
        if idx.size:
            hw = max(hw, int(idx[-1] - idx[0]))
    return hw
