"""The band solver's window sweep, restated in numpy for the tests of both of its forms (tests/test_band_sweeps_host.py,
tests/test_gpu_band_sweeps.py): the matrix families, the np.longdouble reference, the two elimination orders in any dtype and
the entrywise bounds the device is held to.  No GPU.

The sweep returns logdet(A) and gram = R A^-1 R^T for a band matrix A and right-hand-side rows R.  Its single form eliminates
the block columns (16 pixels each) from the first to the last.  Its two-sided ("twisted") form eliminates the first kend0 block
columns top-down and the last kend1 bottom-up -- the same algorithm on the index-reversed matrix -- and then the separator of
nm = 16 (nbr - 1) rows between them, whose Schur complement is what the two halves leave of it, top + flip(bottom) - A_MM
(A_MM is in both).  In either form the elimination writes A = N N^T: N is the Cholesky factor L in the single form, and in
the twisted form the matrix whose column j is the column the elimination produced for pixel j (lower triangular over the top
columns, upper triangular over the bottom ones, both reaching into the separator rows; lower triangular inside the separator).
Z = N^-1 R^T has one row per eliminated column, gram = Z^T Z and logdet = sum_j log N_jj^2.

Bounds (``bounds``).  Both are of the second kind the tests allow, the measured fallback, with the first-order terms as floor:

    floor, logdet:   gamma_K sum_ij |A^-1|_ij (|N||N|^T)_ij + gamma_n sum_j |log N_jj^2|
    floor, gram_rc:  gamma_K (|X_r|^T |N||N|^T |X_c| + 2 |Z_r|^T |Z_c|),  X = A^-1 R^T

from |dA| <= gamma_K |N||N|^T for a factorisation whose longest sum has K terms.  These first-order forms are those of a
factorisation that divides by the diagonal block; the device (and ``eliminate``, which restates it) multiplies by the explicit
inverse F_k = L_kk^-1 instead, whose error carries the condition of the 16 x 16 block, and sums the Gram matrix over all n
columns.  Neither constant is derived here, so each bound is max(floor, 8 x |float64 eliminate - longdouble reference|) on the
same inputs: the device sums in another order (4-wide MFMA chains) but performs the same operations.  Nothing of either bound
comes from the device.  The float64 elimination's own error over the floor is returned too, so that the tests can print how
far the floor alone would have carried."""
import numpy as np

import band_selinv_reference as BS
from band_selinv_reference import BB, LD, gamma

FAMILIES = ("dominant", "matern")
BATCH = 3
# (n, w, nrhs, matern length scale in km/s or None, forms).  nbr = max(3, (w + 31) // 16) window blocks, nblk = n / 16:
#   288/0/1    nbr 3, nblk 18 = 6 nbr: a diagonal matrix at the production edge     288/17/9   8 waves
#   304/16/1   odd split, kend0 = 8, kend1 = 9          128/17/5   nblk 8 = 3 nbr - 1, the smallest that fits: twisted only
#   384/33/17  nbr 4, two blocks of right-hand sides    480/49/33  nbr 5, three blocks, 12 waves
#   784/100/48 nbr 8, the largest nrhs                  864/128/32 nbr 9, 16 waves, two blocks
#   960/144/16 nbr 10, the widest window                992/144/7  odd split at the widest window
#   960/130/2  half-width no multiple of 16             464/144/3  nblk 29 = 3 nbr - 1 at the widest window: twisted only
SHAPES = (
    (288, 0, 1, None, (0, 1)), (288, 17, 9, None, (0, 1)), (304, 16, 1, None, (0, 1)), (128, 17, 5, None, (1,)),
    (384, 33, 17, 2.5, (0, 1)), (480, 49, 33, None, (0, 1)), (784, 100, 48, 8.0, (0, 1)), (864, 128, 32, 10.6, (0, 1)),
    (960, 144, 16, 12.0, (0, 1)), (992, 144, 7, None, (0, 1)), (960, 130, 2, None, (0, 1)), (464, 144, 3, None, (1,)),
)
CASES = [(fam, n, w, nrhs) for n, w, nrhs, ls, _ in SHAPES for fam in FAMILIES if fam == "dominant" or ls is not None]
FORMS = {(n, w, nrhs): forms for n, w, nrhs, _, forms in SHAPES}
_LS = {(n, w, nrhs): ls for n, w, nrhs, ls, _ in SHAPES}
_NEIGHBOUR_LS = (1.0, 0.95, 0.9)  # the batch's matrices 1 and 2: the same kernel, a little narrower


# ------------------------------------------------------------------------------------------ shapes (sf_band_shape.h)
def nbr_of(w):
    return max(3, (w + 2 * BB - 1) // BB)


def twist_shape(n, w):
    """(nm, kend0, kend1, fits) of sfb_twist_shape / sfb_twist_fits for n = 16 nblk."""
    assert n % BB == 0
    nblk, nbr = n // BB, nbr_of(w)
    kend0 = (nblk - (nbr - 1)) // 2
    return (nbr - 1) * BB, kend0, nblk - (nbr - 1) - kend0, nblk >= 2 * nbr + (nbr - 1)


def longest_sum(w, form):
    """K of gamma_K.  An entry of the window takes one product per earlier column that reaches it, fewer than the window's
    16 nbr rows, then the scaling by the pivot's inverse square root and the product with F_k: 16 nbr + 2.  An entry of the
    separator takes at most w + 1 products from the two halves together (a top column c reaches row i only if c >= i - w, a
    bottom column only if c <= j + w, and the separator has nm >= w rows), two additions in the merge, each over at most
    four times |N||N|^T, then up to nm - 1 products in the separator's own sweep: 16 nbr + nm + 10 covers them."""
    nbr = nbr_of(w)
    return BB * nbr + 2 if form == 0 else BB * nbr + (nbr - 1) * BB + 10


# ------------------------------------------------------------------------------------------ matrix families
def dominant(rng, n, w):
    """(A, band, ldb): strictly diagonally dominant, random off-diagonals (band_selinv_reference.band_spd)."""
    return BS.band_spd(rng, n, w)


def matern(n, w, ls):
    """(A, band, ldb): the project's tapered Matern-3/2 kernel on make_order(N=n)'s wavelength grid at amplitude 1e4 and
    length scale ``ls`` km/s (on this grid the taper ends at 12 ls pixels), plus the identity: positive definite by
    construction, conditioned as the workload is (3e3 at ls = 2.5 to 4e5 at ls = 12)."""
    from oracle import sf_oracle as O
    from starfish_amd import synth

    wave = synth.make_order(N=n)["wave"]
    A = O.matern32_global(wave, 1e4, ls) + np.eye(n)
    ii, jj = np.nonzero(A)
    assert np.abs(ii - jj).max() <= w, (n, w, ls, np.abs(ii - jj).max())
    ldb = w + 1 + (w + 1) % 2
    return A, BS.lower_band(A, w, ldb), ldb


# ------------------------------------------------------------------------------------------ reference
def cholesky_band(A):
    """band_selinv_reference.cholesky with every sum cut to the band of A: the same operations in the same order, without
    the products whose factor is a structural zero (a seventh of the time at n = 960, w = 144)."""
    n = A.shape[0]
    ii, jj = np.nonzero(A)
    w = int(np.abs(ii - jj).max())
    L = np.zeros_like(A)
    for j in range(n):
        lo, hi = max(0, j - w), min(n, j + w + 1)
        L[j, j] = np.sqrt(A[j, j] - L[j, lo:j] @ L[j, lo:j])
        L[j + 1:hi, j] = (A[j + 1:hi, j] - L[j + 1:hi, lo:j] @ L[j, lo:j]) / L[j, j]
    return L


def reference(A, rhs):
    """np.longdouble logdet, gram = R A^-1 R^T, L, Z = L^-1 R^T and X = A^-1 R^T of the float64 matrix A and rows rhs."""
    L = cholesky_band(A.astype(LD))
    Z = BS.solve_lower(L, rhs.T.astype(LD))
    X = BS.solve_lower(L, Z, transpose=True)
    return dict(logdet=2 * np.sum(np.log(np.diag(L))), gram=Z.T @ Z, L=L, Z=Z, X=X)


def _sweep(M, R, kend, nb1, N, Zout, col_of):
    """Eliminate the first ``kend`` block columns of the symmetric M (lower triangle used, overwritten with the Schur
    complements) and of the rows R, nb1 blocks below the diagonal: the device's step, L_kk, F = L_kk^-1, X = P F^T, trailing
    update.  Column j of the factor goes to N[rows, col_of(j)], the forward-substituted rows to Zout[col_of(j)]; returns the
    sum of log(pivot)."""
    nblk = M.shape[0] // BB
    sl = lambda k: slice(k * BB, (k + 1) * BB)  # noqa: E731
    logdet = M.dtype.type(0)
    for k in range(kend):
        cnt = min(nb1, nblk - 1 - k)
        Lkk = BS.cholesky(M[sl(k), sl(k)])
        F = BS.inverse_lower(Lkk)
        logdet = logdet + np.sum(np.log(np.diag(Lkk) ** 2))
        rows = slice((k + 1) * BB, (k + 1 + cnt) * BB)
        P = M[rows, sl(k)] @ F.T
        Zk = R[:, sl(k)] @ F.T
        cols = col_of(np.arange(k * BB, (k + 1) * BB))
        N[col_of(np.arange(k * BB, rows.stop))[:, None], cols[None, :]] = np.vstack([Lkk, P])
        Zout[cols] = Zk.T
        M[rows, rows] -= P @ P.T
        R[:, rows] -= Zk @ P.T
    return logdet


def eliminate(A, rhs, w, form, dtype=np.float64):
    """The sweep of ``form`` (0 single, 1 twisted) in ``dtype``: dict(logdet, gram, N, Z), A = N N^T (module docstring) with
    N in the caller's rows and columns and Z = N^-1 R^T, row j from column j.  n must be whole blocks."""
    n, nb1 = A.shape[0], nbr_of(w) - 1
    assert n % BB == 0
    A, rhs = A.astype(dtype), rhs.astype(dtype)
    N, Z = np.zeros((n, n), dtype=dtype), np.zeros((n, rhs.shape[0]), dtype=dtype)
    same = lambda j: j  # noqa: E731
    if form == 0:
        logdet = _sweep(A.copy(), rhs.copy(), n // BB, nb1, N, Z, same)
        return dict(logdet=logdet, gram=Z.T @ Z, N=N, Z=Z)
    nm, kend0, kend1, fits = twist_shape(n, w)
    assert fits
    flip = lambda j: n - 1 - j  # noqa: E731
    top, rtop = A.copy(), rhs.copy()
    bot, rbot = A[::-1, ::-1].copy(), rhs[:, ::-1].copy()
    logdet = _sweep(top, rtop, kend0, nb1, N, Z, same) + _sweep(bot, rbot, kend1, nb1, N, Z, flip)
    gram = Z.T @ Z  # (the two partial Gram matrices: the separator's rows of Z are still zero)
    r0 = kend0 * BB
    sep = slice(r0, r0 + nm)
    M = top[sep, sep] + bot[::-1, ::-1][sep, sep] - A[sep, sep]
    Rm = rtop[:, sep] + rbot[:, ::-1][:, sep] - rhs[:, sep]
    Ns, Zs = np.zeros((nm, nm), dtype=dtype), np.zeros((nm, rhs.shape[0]), dtype=dtype)
    logdet = logdet + _sweep(M, Rm, nm // BB, nb1, Ns, Zs, same)
    N[sep, sep], Z[sep] = Ns, Zs
    return dict(logdet=logdet, gram=gram + Zs.T @ Zs, N=N, Z=Z)


def abs_inverse(ref):
    """|A^-1| in float64 from the reference factor (LAPACK dpotri), kept with the reference: both forms' bounds use it."""
    if "abs_inverse" not in ref:
        from scipy.linalg.lapack import dpotri

        inv, info = dpotri(ref["L"].astype(np.float64), lower=1)
        assert info == 0
        ref["abs_inverse"] = np.abs(np.tril(inv) + np.tril(inv, -1).T)
    return ref["abs_inverse"]


def bounds(ref, A, rhs, w, form, twisted=None):
    """dict(logdet, gram, floor_logdet, floor_gram, cpu_logdet, cpu_gram) for the sweep of ``form``: the bounds of the module
    docstring (max of the first-order floor and eight times the float64 elimination's own error), the floors, and that
    error.  ``ref`` = reference(A, rhs); ``twisted`` = eliminate(A, rhs, w, 1, LD), whose N and Z the floor of form 1 uses.
    The products of the bound itself are float64."""
    n = A.shape[0]
    fac = dict(N=ref["L"], Z=ref["Z"]) if form == 0 else twisted
    aN, aZ = np.abs(fac["N"].astype(np.float64)), np.abs(fac["Z"].astype(np.float64))
    aX = np.abs(ref["X"].astype(np.float64))
    S = aN @ aN.T
    K = longest_sum(w, form)
    diag = np.diag(fac["N"]).astype(np.float64)
    floor_logdet = gamma(K) * np.sum(abs_inverse(ref) * S) + gamma(n) * np.sum(np.abs(np.log(diag ** 2)))
    floor_gram = gamma(K) * (aX.T @ S @ aX + 2 * aZ.T @ aZ)
    cpu = eliminate(A, rhs, w, form, np.float64)
    cpu_logdet = float(abs(LD(cpu["logdet"]) - ref["logdet"]))
    cpu_gram = np.abs(cpu["gram"].astype(LD) - ref["gram"]).astype(np.float64)
    return dict(logdet=max(floor_logdet, 8 * cpu_logdet), gram=np.maximum(floor_gram, 8 * cpu_gram), floor_logdet=floor_logdet,
                floor_gram=floor_gram, cpu_logdet=cpu_logdet, cpu_gram=cpu_gram)


# ------------------------------------------------------------------------------------------ cases, made once
_CASES = {}


def case(family, n, w, nrhs):
    """The batch of a case: dict(A, bands (BATCH, n, ldb), ldb, rhs (BATCH, nrhs, n), forms) plus, through ``checked``, the
    references and bounds of its matrices.  Made once per process, never written."""
    key = (family, n, w, nrhs)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * n + 10 * w + nrhs)
        if family == "dominant":
            mats = [dominant(rng, n, w) for _ in range(BATCH)]
        else:
            mats = [matern(n, w, _LS[n, w, nrhs] * f) for f in _NEIGHBOUR_LS]
        _CASES[key] = dict(A=[m[0] for m in mats], bands=np.stack([m[1] for m in mats]), ldb=mats[0][2], w=w,
                           rhs=rng.standard_normal((BATCH, nrhs, n)), forms=FORMS.get((n, w, nrhs), (0, 1)), checked={})
    return _CASES[key]


def checked(c, b):
    """dict(ref, bounds={form: ...}) of matrix b of case c."""
    if b not in c["checked"]:
        A, rhs, w = c["A"][b], c["rhs"][b], c["w"]
        ref = reference(A, rhs)
        tw = eliminate(A, rhs, w, 1, LD) if 1 in c["forms"] else None
        c["checked"][b] = dict(ref=ref, twisted=tw, bounds={f: bounds(ref, A, rhs, w, f, tw) for f in c["forms"]})
    return c["checked"][b]
