"""Inputs of the batched Cholesky whose factor is known EXACTLY (host helpers of test_potrf_cases_host.py and
test_gpu_potrf_contract.py; numpy only, no GPU).

L0 is lower triangular with dyadic entries (off the diagonal k / 64 with integer |k| <= 8, on it k / 64 with 64 <= k <= 256).
A = L0 L0^T is then exact in fp64 in any order of summation, with or without FMA (every product is a multiple of 2^-12, every
partial sum stays below 2^18 up to n = 16384), and the Cholesky factor of A is L0 itself: pivots are squares of dyadics and
the quotients are exact.  The reference is the truth, for every matrix of a batch, and a dropped or misplaced term of a
kernel's sums is at least 2^-12 (or exactly zero where an integer is 0).  Off-diagonal entries up to 64 / 64 would make A
numerically indefinite from n = 832 on: the range stays at 8 / 64."""
import functools
from collections import namedtuple

import numpy as np

Q = 64          # entries are integers / Q
OFF_RANGE = 8   # |k| of an off-diagonal entry
GUARD_ROWS = 64  # virtual rows of the shifted frame (sf_potrf_front_pad): the front guard covers them

# (n, batch): the sizes at which the launch sequences take another path
SHAPES = [
    (64, 1),    # one leaf
    (128, 3),   # one panel
    (192, 3),   # 64 mod 128, below the size from which the frame is shifted
    (320, 3),   # the smallest shifted frame
    (768, 17),  # six panels: a wide pair with A(p) and both B groups, then the narrow tail; split-K 2 and 4; batch >= 16
    (832, 9),   # shifted to seven panels: odd count, trailing single panel; batch no multiple of the 8 dataflow queues
    (1216, 3),  # shifted to ten panels; split-K 8 from column 1024
]
# pivot failures (test 4): batch 5, matrices 1 and 4 fail; tile edges of the plain (768) and of the shifted frame (832)
PIVOT_BATCH = 5
PIVOTS = {
    768: [0, 63, 64, 127, 128, 255, 256, 511, 640, 767],
    832: [0, 63, 64, 127, 128, 255, 256, 511, 640, 831, 191, 192, 319, 320],
}


def pivot_pairs(n):
    """Two failing columns per run: (p of matrix 1, p of matrix 4)."""
    p = PIVOTS[n]
    return [(p[i], p[i + 1]) for i in range(0, len(p), 2)]


def dyadic_factor(rng, n):
    L0 = np.tril(rng.integers(-OFF_RANGE, OFF_RANGE + 1, size=(n, n)), -1).astype(np.float64)
    L0[np.arange(n), np.arange(n)] = rng.integers(Q, 4 * Q + 1, size=n)
    return L0 / Q


def spd_of(L0):
    return L0 @ L0.T


def not_pd_at(A, L0, p):
    """A - (L0[p, p]^2 + 1) e_p e_p^T (exact): the Schur pivot p is -1, every earlier pivot and column is untouched."""
    out = A.copy()
    out[p, p] -= L0[p, p] ** 2 + 1.0
    return out


@functools.lru_cache(maxsize=None)
def case(n, batch, seed=0):
    """(L0[batch, n, n], A[batch, n, n]) of a shape; computed once and shared -- callers must not write into them."""
    rng = np.random.default_rng([n, batch, seed])
    L0 = np.stack([dyadic_factor(rng, n) for _ in range(batch)])
    A = np.stack([spd_of(L) for L in L0])
    L0.setflags(write=False)
    A.setflags(write=False)
    return L0, A


Layout = namedtuple("Layout", "name n lda stride")


def layouts(n):
    return [Layout("tight", n, n, n * n), Layout("padded", n, n + 16, n * (n + 16) + 2 * (n + 16))]


class Embedded:
    """`batch` matrices inside one flat buffer of doubles that is NaN wherever no matrix entry lies: `front` doubles before
    matrix 0, the columns n .. lda of every row, the gap between two matrices and `rear` doubles behind the last one."""

    def __init__(self, buf, layout, batch, front):
        self.buf, self.layout, self.batch, self.front = buf, layout, batch, front

    def matrices(self, buf=None):
        """Strided (batch, n, n) view of the matrices of `buf` (numpy array of the same length; default: the buffer)."""
        buf = self.buf if buf is None else buf
        L = self.layout
        return np.lib.stride_tricks.as_strided(buf[self.front:], shape=(self.batch, L.n, L.n),
                                               strides=(8 * L.stride, 8 * L.lda, 8))

    def outside_is_nan(self, buf):
        """True when every double of `buf` that is no matrix entry is (still) NaN."""
        probe = np.array(buf, copy=True)
        self.matrices(probe)[...] = 0.0
        return int(np.isnan(probe).sum()) == probe.size - self.batch * self.layout.n ** 2


def embed(A_batch, layout, upper="sym", front=None):
    """upper: "sym" keeps the strict upper triangle of A_batch as given, "nan" poisons it (diagonal tiles included)."""
    A_batch = np.asarray(A_batch, dtype=np.float64)
    batch, n = A_batch.shape[0], layout.n
    assert A_batch.shape == (batch, n, n) and upper in ("sym", "nan")
    min_front = GUARD_ROWS * (layout.lda + 1)
    front = min_front if front is None else front
    assert front >= min_front and front % 2 == 0  # (matrix 0 keeps the 16-byte alignment of the allocation)
    rear = GUARD_ROWS * layout.lda + 4096
    buf = np.full(front + batch * layout.stride + rear, np.nan)
    e = Embedded(buf, layout, batch, front)
    M = e.matrices()
    M[...] = A_batch
    if upper == "nan":
        iu = np.triu_indices(n, 1)
        M[:, iu[0], iu[1]] = np.nan
    return e


def blocked_cholesky(A, nb=128, kc=16, skip=None):
    """numpy emulation of the library's algorithm: left-looking panels of nb columns, the diagonal tile factorised on its own,
    the rows below as T inv(L_kk)^T with the EXPLICIT inverse, T = A_ik - sum over kc-wide K chunks of L_i. L_k.^T.
    skip = (i, k, c): chunk c (columns c kc .. c kc + kc) is left out of the update of tile (i, k) -- the fault the GPU tests
    must be able to see."""
    import scipy.linalg

    n = A.shape[0]
    L = np.zeros_like(A)
    for k0 in range(0, n, nb):
        k1 = min(k0 + nb, n)
        D = A[k0:k1, k0:k1] - L[k0:k1, :k0] @ L[k0:k1, :k0].T
        Lkk = np.linalg.cholesky(D)
        W = scipy.linalg.solve_triangular(Lkk, np.eye(k1 - k0), lower=True)
        L[k0:k1, k0:k1] = Lkk
        for i0 in range(k1, n, nb):
            i1 = min(i0 + nb, n)
            T = A[i0:i1, k0:k1] - L[i0:i1, :k0] @ L[k0:k1, :k0].T
            if skip is not None and (i0 // nb, k0 // nb) == tuple(skip[:2]):
                c0 = skip[2] * kc
                assert c0 + kc <= k0
                T += L[i0:i1, c0:c0 + kc] @ L[k0:k1, c0:c0 + kc].T
            L[i0:i1, k0:k1] = T @ W.T
    return L


# ---- sf_logdet_sqmah_batch on given factors (test 5) -----------------------------------------------------------------------
def solve_case(n, batch, seed=0):
    """L0[batch, n, n], z0[batch, n] dyadic (k / 64, |k| <= 64), R = L0 z0 (exact), and the known results
    logdet = 2 sum log L0_kk (long double) and sqmah = sum z0^2 (exact)."""
    rng = np.random.default_rng([n, batch, seed, 5])
    L0 = np.stack([dyadic_factor(rng, n) for _ in range(batch)])
    z0 = rng.integers(-Q, Q + 1, size=(batch, n)) / Q
    R = np.einsum("bij,bj->bi", L0, z0)
    return L0, z0, R, logdet_of(np.diagonal(L0, axis1=1, axis2=2)), (z0 * z0).sum(axis=1)


def logdet_of(diag):
    return np.array(2.0 * np.log(np.asarray(diag, dtype=np.longdouble)).sum(axis=-1), dtype=np.float64)
