"""Cases and CPU references for the transform-chain tests (tests/test_gpu_transform_chain.py,
tests/test_transform_reference.py): orders that hit a requested FFT length nf, walker batches that reach the
size-dependent branches of sf_transform_batch (emulator -> rotational broadening -> spline fit -> Doppler-shifted spline
evaluation -> Chebyshev / extinction -> scale), and tolerances derived from error bounds instead of fixed constants:

* ``rot_mult_bound``   per-bin bound on the fp64 error of the Gray rotational kernel, which cancels catastrophically for
                       small u (terms of size 3 / (2 u^2) that sum to ~1);
* ``ainv_norm``        ||A^-1||_inf of the quintic collocation matrix of a grid (A is totally positive, so A^-1 has a
                       checkerboard sign pattern and one banded solve against (-1)^j gives the norm exactly);
* ``lebesgue``         sum_j |B_j(x)| at each query: 1 inside the knot range, the growth of the end pieces outside it;
* ``chain_reference``  the oracle's (flux, X, scale) of one walker and per-pixel tolerances: the per-bin bound pushed
                       through the irfft, ||A^-1||_inf, the Lebesgue factor and the reconstruction, plus a floor of
                       1e-10 max|flux| (the repository's usual tolerance) scaled by the Lebesgue factor."""
import functools
from math import pi

import numpy as np
from scipy.linalg import solve_banded

from oracle import sf_oracle as O
from starfish_amd import synth

EPS = np.finfo(np.float64).eps
C_ROT = 4.0  # rot_mult_bound's constant: the measured worst case of scipy's j1 / numpy's cos, sin is 1.02 (u in [1e-5, 10])
FLOOR = 1e-10  # relative floor of every flux / X comparison (the repository's transform parity tolerance)
LDS_FFT_MAX = 8192  # complex points that sf_transform_fft.h (kLdsFftMax) keeps in LDS
NF_MIN_VSINI, NF_MAX_VSINI = 16, 65536  # FFT lengths the broadened model accepts
DV = 2.0  # km/s, pixel spacing of every synthetic order here
VZ_FAR = 1500.0  # km/s: shifts a synthetic order by 750 pixels


# ------------------------------------------------------------------------------------------------ orders
def branch(nf):
    """The kernel path an FFT length takes.  Hot path (k_broaden_half + sf_fft_inplace_r4): a half-size transform of
    L = nf / 2 points, in LDS iff L <= 8192, with a plain radix-2 pre-pass iff log2(L) is odd.  Free functions
    (k_broaden<true, *>): the full-length transform, in LDS iff nf <= 8192."""
    L = nf // 2
    stages = L.bit_length() - 1
    return dict(L=L, half_lds=L <= LDS_FFT_MAX, half_odd=bool(stages & 1), full_lds=nf <= LDS_FFT_MAX)


def default_pad_steps(nf):
    """Padding (in pixels of DV) of the emulator grid on each side of the data: one pixel at the smallest nf, 745 from
    nf = 16384 on (VZ_FAR then moves 5 pixels past the end of the grid)."""
    return int(min(max(1, nf // 16), 745))


def make_nf_order(nf, m=4, seed=0, N=None, pad_steps=None, wave0=5000.0, max_pixels=4096):
    """synth.make_order with N pixels and ``pad_steps`` pixels of padding such that len(min_dv_wave) == nf.  Default
    N fills three quarters of the grid.  Orders of more than ``max_pixels`` pixels keep the first and last 1024 and
    every k-th one in between (a masked order: the transform chain still spans the whole grid, the N x N buffers of
    the batched calls stay small)."""
    if pad_steps is None:
        pad_steps = default_pad_steps(nf)
    if N is None:
        N = max(6, int(0.75 * nf) - 2 * pad_steps)
    pad = pad_steps * wave0 * DV / synth.C_KMS
    o = dict(synth.make_order(N=N, m=m, seed=seed, dv=DV, wave0=wave0, pad=pad))
    assert len(o["emu_wl"]) == nf, (nf, N, pad_steps, len(o["emu_wl"]))
    if N > max_pixels:
        stride = -(-(N - 2048) // (max_pixels - 2048))
        keep = np.zeros(N, dtype=bool)
        keep[:1024] = keep[-1024:] = True
        keep[1024:-1024:stride] = True
        for k in ("wave", "flux", "sigma"):
            o[k] = o[k][keep]
    return o


def oracle_order(o):
    oo = O.OracleOrder(o["wave"], o["flux"], o["sigma"], o["emu_wl"], o["eigenspectra"], o["flux_mean"],
                       o["flux_std"], o["grid_points"], o["w_hat"])
    return oo


# ------------------------------------------------------------------------------------------------ walkers
VSINIS = (0.5, 2.0, 30.0, 300.0)  # 300 km/s takes the kernel past its first zero at every nf here
VZS = (0.0, 10.0, -10.0)


def walker(k, vsini=True, vz=True, log_scale=True, n_cheb=2, av=False, far=False):
    """Walker k: vsini cycles through VSINIS, vz through VZS (or +-VZ_FAR on every fourth walker when ``far``), each
    value offset slightly per walker so that no two walkers of a batch agree."""
    j = k // 4
    p = dict(grid=[6010.0 + 7.0 * (k % 23), 4.1 + 0.031 * (k % 19), -0.9 + 0.047 * (k % 17)])
    if vsini:
        p["vsini"] = VSINIS[k % 4] * (1 + 0.003 * j)
    if vz:
        if far and k % 4 == 1:
            p["vz"] = VZ_FAR * (1 if j % 2 == 0 else -1) + 0.1 * j
        else:
            p["vz"] = VZS[k % 3] + 0.01 * j
    if log_scale:
        p["log_scale"] = 0.01 * (k % 7) - 0.02
    if n_cheb:
        p["cheb"] = [0.01 - 0.001 * (k % 5), -0.02 + 0.002 * (k % 3), 0.003][:n_cheb]
    if av:
        p["Av"] = 0.2 + 0.05 * (k % 6)
    return p


def walkers(B, **kw):
    return [walker(k, **kw) for k in range(B)]


def pixels_outside(oo, vz):
    """Data pixels that the Doppler shift by vz moves outside the knot range [t[5] s, t[nf] s] of min_dv_wave."""
    s = np.sqrt((O.C_KMS + vz) / (O.C_KMS - vz))
    w = oo.min_dv_wave
    return int(np.sum((oo.wave < w[0] * s) | (oo.wave > w[-1] * s)))


# ------------------------------------------------------------------------------------------------ bounds
def gray_mult(u):
    """The reference's Gray kernel at u > 0 (transforms.py:129-131), in fp64 as the oracle evaluates it."""
    from scipy.special import j1

    return j1(u) / u - 3 * np.cos(u) / (2 * u**2) + 3.0 * np.sin(u) / (2 * u**3)


def rot_mult_bound(u):
    """Bound on |gray_mult(u) - exact| for fp64 evaluation: C_ROT eps (1 + 3 / u^2).  The cancelling terms are of size
    3 / (2 u^2); each carries a few roundings."""
    u = np.asarray(u, dtype=np.float64)
    return C_ROT * EPS * (1 + 3 / u**2)


def inst_mult_bound(a2):
    """Bound on the fp64 error of exp(-2 a^2) (a = pi sigma freq): the argument's relative rounding (a few eps)
    times its size, plus the rounding of exp itself."""
    a2 = np.asarray(a2, dtype=np.float64)
    return 8 * EPS * (1 + 2 * a2) * np.exp(-2 * a2)


def irfft_bound(spec, mult_bound):
    """Bound on the change of irfft(spec * mult) when every multiplier k > 0 moves by at most mult_bound[k - 1]:
    (2 / nf) sum_k bound_k |X_k| per row (the DC bin is multiplied by exactly 1)."""
    nf = 2 * (spec.shape[-1] - 1)
    return 2.0 / nf * np.sum(mult_bound * np.abs(spec[..., 1:]), axis=-1)


def collocation_banded(x):
    """The quintic collocation matrix of grid x in solve_banded's (5, 5) storage."""
    ab, offs, _ = O.quintic_collocation_band(x)
    n = len(x)
    band = np.zeros((11, n))
    for i in range(n):
        for q in range(6):
            j = offs[i] + q
            band[5 + i - j, j] = ab[i, q]
    return band


def collocation_dense(x):
    ab, offs, _ = O.quintic_collocation_band(x)
    n = len(x)
    A = np.zeros((n, n))
    for i in range(n):
        A[i, offs[i] : offs[i] + 6] = ab[i]
    return A


@functools.lru_cache(maxsize=None)
def _ainv_norm_cached(key):
    x = np.frombuffer(key, dtype=np.float64)
    s = (-1.0) ** np.arange(len(x))
    return float(np.max(np.abs(solve_banded((5, 5), collocation_banded(x), s))))


def ainv_norm(x):
    """||A^-1||_inf of the quintic collocation matrix of grid x.  A is totally positive, so (A^-1)_ij (-1)^(i+j) >= 0
    and the largest absolute row sum of A^-1 is max_i |(A^-1 s)_i| with s_j = (-1)^j (test_transform_reference.py
    checks this against the dense inverse)."""
    return _ainv_norm_cached(np.ascontiguousarray(x, dtype=np.float64).tobytes())


K_EXACT = 256  # bins whose spline-fit amplification amp_of_bins computes exactly


@functools.lru_cache(maxsize=None)
def _amp_cached(key):
    x = np.frombuffer(key, dtype=np.float64)
    n = len(x)
    K = min(K_EXACT, n // 2 + 1)
    j = np.arange(n)[:, None]
    th = 2 * pi * np.arange(1, K + 1)[None, :] / n
    sol = solve_banded((5, 5), collocation_banded(x), np.hstack([np.cos(th * j), np.sin(th * j)]))
    amp = np.full(n // 2, ainv_norm(x))
    amp[: min(K, n // 2)] = np.max(np.hypot(sol[:, :K], sol[:, K:]), axis=0)[: min(K, n // 2)]
    return np.minimum(amp, ainv_norm(x))


def amp_of_bins(x):
    """a_k, k = 1 .. n/2: max over the phase phi and the rows i of |(A^-1 cos(2 pi k j / n + phi))_i|, i.e.
    max_i hypot((A^-1 c_k)_i, (A^-1 s_k)_i), exactly for k <= K_EXACT and ||A^-1||_inf above (a smooth error passes
    the interpolation almost unchanged, an alternating one is amplified by up to ||A^-1||_inf)."""
    return _amp_cached(np.ascontiguousarray(x, dtype=np.float64).tobytes())


def lebesgue(t, ncoef, xq):
    """sum_j |B_j(x)| of the spline's six B-splines at every query x (interval search of splev, clamped to the end
    pieces): exactly 1 inside [t[5], t[ncoef]], the growth of the extrapolated end pieces outside."""
    xq = np.asarray(xq, dtype=np.float64)
    lam = np.ones(len(xq))
    for q in np.nonzero((xq < t[5]) | (xq > t[ncoef]))[0]:
        ell = O.find_interval(t, ncoef, xq[q])
        lam[q] = np.sum(np.abs(O.bspline_basis6(t, ell, xq[q])))
    return lam


def resample_tol(x, y, xq, c=64.0):
    """Per-query tolerance of the k = 5 interpolating spline against FITPACK: c eps cond(A) max|y| times the Lebesgue
    factor of the query (cond(A) = ||A||_inf ||A^-1||_inf of the dense collocation matrix; ||A||_inf = 1)."""
    A = collocation_dense(x)
    cond = np.abs(A).sum(axis=1).max() * np.abs(np.linalg.inv(A)).sum(axis=1).max()
    lam = lebesgue(O.quintic_knots(x), len(x), xq)
    return c * EPS * cond * np.max(np.abs(y)) * lam


# ------------------------------------------------------------------------------------------------ the chain
def chain_reference(oo, p):
    """The oracle's (flux, X, scale) of walker p (O.emulator_terms) and per-pixel tolerances tol_flux (N,), tol_X (m, N)
    for the device's values:
      coefs  ec_r  = 2 (2 / nf) sum_k rot_mult_bound(u_k) a_k |X_rk|  (device and oracle each within the bound; a_k the
                     spline fit's amplification of bin k, amp_of_bins)
      pixel  E_ri  = Lebesgue_i (ec_r + FLOOR max|R_r|)
    propagated through X_k = scale g^2 R_k R_std and flux = scale (g^2 sum_k w_k R_k R_std + g R_mean) (g: Chebyshev
    times extinction), plus FLOOR max|.| Lebesgue_i on X and flux, then through the renormalised scale when log_scale
    is absent.  (The row floor grows twice with the Lebesgue factor in the product of two extrapolated rows.)"""
    flux, X, _, scale = O.emulator_terms(oo, p)
    wave = oo.min_dv_wave
    rows = oo.bulk_fluxes
    nf = rows.shape[1]
    if "vsini" in p:
        dv = O.min_velocity_step(wave)
        u = (2.0 * pi * p["vsini"] * np.fft.rfftfreq(nf, dv))[1:]
        ec = 2 * irfft_bound(np.fft.rfft(rows), rot_mult_bound(u) * amp_of_bins(wave))
        rows = O.rot_broaden(wave, rows, p["vsini"])
    else:
        ec = np.zeros(rows.shape[0])
    s = np.sqrt((O.C_KMS + p["vz"]) / (O.C_KMS - p["vz"])) if "vz" in p else 1.0
    xs = O.doppler(wave, p["vz"]) if "vz" in p else wave
    lam = lebesgue(O.quintic_knots(xs), nf, oo.wave)
    R = O.quintic_resample(xs, rows, oo.wave)
    inside = lam == 1.0
    row_ref = np.max(np.abs(R[:, inside] if inside.any() else R), axis=1)
    E = lam[None, :] * (ec + FLOOR * row_ref)[:, None]
    g = np.ones(len(oo.wave))
    if "Av" in p:
        g = g * O.extinct_ccm89(oo.wave, np.ones(len(oo.wave)), p["Av"])
    if "cheb" in p:
        g = g * O.cheb_correct(oo.wave, np.ones(len(oo.wave)), [1, *p["cheb"]])
    w_mu, _ = O.emulator_query(oo.grid_points, p["grid"], oo.variances, oo.lengthscales, oo.v11, oo.w_hat)
    m = R.shape[0] - 2
    Rk, Rm, Rs = R[:m], R[m], R[m + 1]
    Ek, Em, Es = E[:m], E[m], E[m + 1]
    fu, Xu = flux / scale, X / scale  # unscaled
    ref_f = np.max(np.abs(fu[inside] if inside.any() else fu))
    ref_x = np.max(np.abs(Xu[:, inside] if inside.any() else Xu))
    dXb = g**2 * (Ek * np.abs(Rs) + np.abs(Rk) * Es + Ek * Es)
    dXu = dXb + FLOOR * ref_x * lam[None, :]
    dFu = np.abs(w_mu) @ dXb + np.abs(g) * Em + FLOOR * ref_f * lam
    if "log_scale" in p:
        dscale = 0.0
    else:
        norm = p.get("norm", 1)
        dw = np.abs(np.diff(oo.wave))
        den = abs(O.trapezoid(fu * norm, oo.wave))
        dscale = scale * np.sum(dw * (dFu[1:] + dFu[:-1]) / 2.0) * abs(norm) / den
    tol_flux = scale * dFu + np.abs(fu) * dscale
    tol_X = scale * dXu + np.abs(Xu) * dscale
    tol_log_scale = dscale / scale + 4 * EPS
    return dict(flux=flux, X=X, scale=scale, log_scale=np.log(scale), tol_flux=tol_flux, tol_X=tol_X,
                tol_log_scale=tol_log_scale, lam=lam)


def sensitivity(oo, p, tol_flux):
    """Smallest max_i |flux'_i - flux_i| / tol_i over the perturbations that apply to p: vsini by 1 %, vz by 1 km/s, the
    first Chebyshev coefficient by 1e-3.  A case must be able to see each of them (> 100)."""
    base = O.emulator_terms(oo, p)[0]
    moves = []
    if "vsini" in p:
        moves.append(dict(p, vsini=p["vsini"] * 1.01))
    if "vz" in p:
        moves.append(dict(p, vz=p["vz"] + 1.0))
    if p.get("cheb"):
        moves.append(dict(p, cheb=[p["cheb"][0] + 1e-3, *p["cheb"][1:]]))
    return min(np.max(np.abs(O.emulator_terms(oo, q)[0] - base) / tol_flux) for q in moves)


def broaden_reference(wave, flux, kind, param):
    """O.rot_broaden / O.inst_broaden of the rows of flux and the per-element tolerance of the device's free function:
    the per-bin multiplier bound pushed through the irfft (twice: device and oracle) plus FLOOR max|out|."""
    flux = np.atleast_2d(flux)
    nf = flux.shape[-1]
    dv = O.min_velocity_step(wave)
    freq = np.fft.rfftfreq(nf, dv)
    spec = np.fft.rfft(flux)
    if kind == "rot":
        out = O.rot_broaden(wave, flux, param)
        bnd = rot_mult_bound((2.0 * pi * param * freq)[1:])
    else:
        out = O.inst_broaden(wave, flux, param)
        bnd = inst_mult_bound(((pi * param / 2.355) * freq[1:]) ** 2)
    tol = 2 * irfft_bound(spec, bnd)[:, None] + FLOOR * np.max(np.abs(out))
    return out, np.broadcast_to(tol, out.shape)


def kill_fwhm(nf, dv, k_keep=8):
    """A FWHM whose Gaussian multiplier is exp(-460 (k / k_keep)^2): 1, 7.6e-4, 3e-13, 8e-29 at k = 0 .. 3 for k_keep = 8
    and 1e-200 at k = k_keep -- every bin but the first few is wiped out."""
    sigma = np.sqrt(230.0) * nf * dv / (pi * k_keep)
    return 2.355 * sigma


# ------------------------------------------------------------------------------------------------ the GPU cases
HOT_NFS = (16, 32, 64, 128, 256, 1024, 2048, 4096, 8192, 16384, 32768, 65536)
MS = (1, 14, 15, 30, 31, 32)  # m + 2 = 3, 16 | 17, 32 | 33, 34: one, two and three column blocks of k_spline_apply
BATCH_NFS = (16384, 65536)
BATCHES = (1, 2, 3, 5, 33, 64)
RENORM_PIXELS = (2, 3, 257)
MODEL_VARIANTS = ("plain", "cheb3_av", "av", "no_vz", "no_vsini")


def variant_kw(v):
    return dict(plain=dict(n_cheb=0), cheb3_av=dict(n_cheb=3, av=True), av=dict(n_cheb=0, av=True),
                no_vz=dict(vz=False), no_vsini=dict(vsini=False))[v]


@functools.lru_cache(maxsize=None)
def case_order(kind, key):
    """(order, OracleOrder) of a case.  kind 'nf': make_nf_order(key); 'm': nf = 2048 with m = key; 'pixels': a
    renormalisation order of key pixels (nf = 16, 32 and 512 for 2, 3 and 257)."""
    if kind == "nf":
        o = make_nf_order(key, seed=key % 97)
    elif kind == "m":
        o = make_nf_order(2048, m=key, seed=key)
    elif kind == "pixels":
        if key < 6:
            # the first, (middle,) last of 11 pixels -- far enough apart for a Chebyshev term to survive the
            # renormalisation -- and 50 pixels of padding: the model's grid (spacing: the data's, 10 or 5 pixels) then
            # has 16 or 32 points
            pad = 50 * 5000.0 * DV / synth.C_KMS
            o = dict(synth.make_order(N=11, m=4, seed=key, dv=DV, pad=pad))
            keep = np.linspace(0, 10, key).astype(int)
            for k in ("wave", "flux", "sigma"):
                o[k] = o[k][keep]
        else:
            o = make_nf_order(512, N=key, pad_steps=64, seed=key)
    else:
        raise ValueError(kind)
    return o, oracle_order(o)


def case_walkers(kind, key, B=4, variant=None):
    """Walker dicts of a case.  Orders of nf >= 16384 (745 pixels of padding) get VZ_FAR walkers."""
    if kind == "nf":
        return walkers(B, far=key >= 16384)
    if kind == "m":
        return walkers(3)
    if kind == "pixels":
        return walkers(3, log_scale=False)
    raise ValueError(kind)


def sensitivity_cases():
    """(label, kind, key, walkers) of every GPU case of the chain whose flux the sensitivity check covers; batches of
    more than 12 walkers are represented by their first 12 (every combination of the vsini and vz cycles)."""
    out = [(f"nf{nf}", "nf", nf, case_walkers("nf", nf)) for nf in HOT_NFS]
    out += [(f"nf{nf}-B64", "nf", nf, walkers(12, far=True)) for nf in BATCH_NFS]
    out += [(f"m{m}", "m", m, case_walkers("m", m)) for m in MS]
    out += [(f"px{n}", "pixels", n, case_walkers("pixels", n)) for n in RENORM_PIXELS]
    out += [(f"nf1024-{v}", "nf", 1024, walkers(4, **variant_kw(v))) for v in MODEL_VARIANTS]
    out += [("nf16384-renorm", "nf", 16384, walkers(4, far=True, log_scale=False))]
    return out
