"""sf_potrs_batch alone: the factor left by sf_potrf_batch applied to right-hand sides (L Z, L^-1 B, L^-T B, C^-1 B).

The reference is the downloaded L itself in np.longdouble, so only the new kernels are under test, and the bounds are the
componentwise ones of Higham, Accuracy and Stability of Numerical Algorithms (2nd ed.), Thm 8.5 (substitution) and
Thm 10.4 (Cholesky solve), with u = 2^-53 and gamma_k = k u / (1 - k u): valid for any order of summation, hence for the
MFMA's.  After the factorisation everything above the diagonal -- inside the diagonal tiles too -- is overwritten with
NaN: a single read from there poisons the result."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OPS = {"L": 0, "Linv": 1, "LinvT": 2, "Cinv": 3}
BATCH = 3
U = 2.0 ** -53


def gamma(k):
    return k * U / (1 - k * U)


@pytest.fixture(scope="module")
def gpu():
    import torch

    from starfish_amd import _lib

    lib = _lib.require_gpu()
    return lib, torch.device("cuda", torch.cuda.current_device())


_FACTORS = {}


def factors(gpu, n, lda):
    """(device array (BATCH, n, lda) holding L below and NaN above the diagonal, L as longdouble (BATCH, n, n)); made once
    per shape and never written again."""
    import torch

    from starfish_amd import _device as D, _lib

    if (n, lda) in _FACTORS:
        return _FACTORS[(n, lda)]
    lib, dev = gpu
    rng = np.random.default_rng(1000 * n + lda)
    A = np.zeros((BATCH, n, lda))
    for b in range(BATCH):
        G = rng.standard_normal((n, n))
        A[b, :, :n] = G @ G.T + n * np.eye(n)
    dA = D.to_dev(A, dev)
    info = torch.zeros(BATCH, dtype=torch.int32, device=dev)
    ws = D.workspace(lib.sf_potrf_workspace_bytes(n, BATCH), dev)
    _lib.check(lib.sf_potrf_batch(D.ptr(dA), n, lda, n * lda, BATCH, D.ptr(info), D.ptr(ws), ws.numel(), D.stream_ptr(dev)),
               "sf_potrf_batch")
    torch.cuda.synchronize(dev)
    assert (info.cpu().numpy() == 0).all()
    del ws
    above = torch.arange(lda, device=dev)[None, :] > torch.arange(n, device=dev)[:, None]
    dA[:, above] = float("nan")
    L = np.tril(dA.cpu().numpy()[:, :, :n]).astype(np.longdouble)
    assert np.isfinite(L).all()
    _FACTORS[(n, lda)] = (dA, L)
    return _FACTORS[(n, lda)]


def potrs(gpu, dA, n, lda, op, rhs, nrhs, ldr, rhs_stride, out, ldo, out_stride):
    from starfish_amd import _device as D, _lib

    lib, dev = gpu
    rc = lib.sf_potrs_batch(D.ptr(dA), n, lda, n * lda, BATCH, OPS[op], D.ptr(rhs), nrhs, ldr, rhs_stride, D.ptr(out), ldo,
                            out_stride, D.stream_ptr(dev))
    _lib.check(rc, "sf_potrs_batch")


def check_bound(op, L, x, b, n):
    """x: result, b: right-hand side, both (nrhs, n) of ONE matrix L (longdouble)."""
    X, Bm = x.astype(np.longdouble).T, b.astype(np.longdouble).T  # (n, nrhs)
    aL = np.abs(L)
    g = np.longdouble(gamma(n))
    if op == "L":
        err, bound = np.abs(X - L @ Bm), g * (aL @ np.abs(Bm))
    elif op == "Linv":
        err, bound = np.abs(L @ X - Bm), g * (aL @ np.abs(X))
    elif op == "LinvT":
        err, bound = np.abs(L.T @ X - Bm), g * (aL.T @ np.abs(X))
    else:
        err, bound = np.abs(L @ (L.T @ X) - Bm), (2 * g + g * g) * (aL @ (aL.T @ np.abs(X)))
    worst = float(np.max(err / bound))
    print(f"{op}: n={n} max err / bound = {worst:.3g}")
    assert np.isfinite(x).all()
    assert (err <= bound).all(), (op, n, worst)


@pytest.mark.parametrize("op", list(OPS))
@pytest.mark.parametrize("nrhs", [1, 16, 17])
@pytest.mark.parametrize("lda_pad", [0, 16])
@pytest.mark.parametrize("n", [64, 128, 192, 320])
def test_potrs_within_the_componentwise_bounds_and_reproducible(gpu, n, lda_pad, nrhs, op):
    import torch

    from starfish_amd import _device as D

    lib, dev = gpu
    lda = n + lda_pad
    dA, L = factors(gpu, n, lda)
    ldr = n + (1 if nrhs == 17 else 0)  # (an odd row stride: the 8-byte loads)
    rng = np.random.default_rng(7 * n + 3 * nrhs + lda_pad + OPS[op])
    B = np.zeros((BATCH, nrhs, ldr))
    B[:, :, :n] = rng.standard_normal((BATCH, nrhs, n))
    dB = D.to_dev(B, dev)
    # out of place, into a buffer with NaN between the rows' ends and the next row
    out = torch.full((BATCH, nrhs, ldr), float("nan"), dtype=torch.float64, device=dev)
    potrs(gpu, dA, n, lda, op, dB, nrhs, ldr, nrhs * ldr, out, ldr, nrhs * ldr)
    got = out.cpu().numpy()
    if ldr > n:
        assert np.isnan(got[:, :, n:]).all()  # nothing written behind the n rows
    for b in range(BATCH):
        check_bound(op, L[b], got[b, :, :n], B[b, :, :n], n)
    # in place: the same bits
    inplace = dB.clone()
    potrs(gpu, dA, n, lda, op, inplace, nrhs, ldr, nrhs * ldr, inplace, ldr, nrhs * ldr)
    np.testing.assert_array_equal(inplace.cpu().numpy()[:, :, :n], got[:, :, :n])
    # one block shared by every matrix (rhs_stride 0) == a copy of that block per matrix
    shared = torch.empty((BATCH, nrhs, ldr), dtype=torch.float64, device=dev)
    potrs(gpu, dA, n, lda, op, dB[0].contiguous(), nrhs, ldr, 0, shared, ldr, nrhs * ldr)
    copies = torch.empty((BATCH, nrhs, ldr), dtype=torch.float64, device=dev)
    potrs(gpu, dA, n, lda, op, dB[0:1].repeat(BATCH, 1, 1).contiguous(), nrhs, ldr, nrhs * ldr, copies, ldr, nrhs * ldr)
    np.testing.assert_array_equal(shared.cpu().numpy()[:, :, :n], copies.cpu().numpy()[:, :, :n])
    np.testing.assert_array_equal(shared.cpu().numpy()[0, :, :n], got[0, :, :n])
    # the factor was only read
    assert torch.equal(torch.tril(dA[:, :, :n]).cpu(), torch.from_numpy(L.astype(np.float64)))
