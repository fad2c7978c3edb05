"""sf_potri_diag_batch alone: diag(C^-1) = the squared column norms of X = L^-1 for the L left by sf_potrf_batch.

The reference is the downloaded L itself, inverted by substitution in np.longdouble, so only the new kernels are under test.
Bound, componentwise, with u = 2^-53 and gamma_k = k u / (1 - k u):
    |d^ - d| <= 2 gamma_2n diag(|X|^T |X| |L| |X|) + gamma_{n+1} d.
The first-order forward error of a triangular inverse is |dX| <= gamma |X||L||X| whether the computed inverse satisfies a
left or a right residual bound (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., ch. 14); the constant is
2n to cover a product with a computed block inverse on top of the long sum; d = sum X^2 turns dX into 2 |X|^T |dX|, and the
second term is the sum of squares itself.  Before the call everything above the diagonal -- inside the diagonal blocks
too -- is overwritten with NaN: a single read from there before it is written poisons the result."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BATCH = 3
U = 2.0 ** -53
SF_EINVAL = -1


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
    per shape and never written again: the tests work on clones."""
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
    dA[:, above_diagonal(n, lda, dev)] = float("nan")
    L = np.tril(dA.cpu().numpy()[:, :, :n]).astype(np.longdouble)
    assert np.isfinite(L).all()
    _FACTORS[(n, lda)] = (dA, L)
    return _FACTORS[(n, lda)]


def above_diagonal(n, lda, dev):
    import torch

    return torch.arange(lda, device=dev)[None, :] > torch.arange(n, device=dev)[:, None]


def inverse_longdouble(L):
    """X = L^-1 by forward substitution, row by row, in the precision of L."""
    n = L.shape[0]
    X = np.zeros_like(L)
    for i in range(n):
        row = -(L[i, :i] @ X[:i])
        row[i] += 1
        X[i] = row / L[i, i]
    return X


def potri_diag(gpu, dA, n, lda, out, out_stride, ws=None):
    from starfish_amd import _device as D, _lib

    lib, dev = gpu
    if ws is None:
        ws = D.workspace(lib.sf_potri_diag_workspace_bytes(n, BATCH), dev)
    rc = lib.sf_potri_diag_batch(D.ptr(dA), n, lda, n * lda, BATCH, D.ptr(out), out_stride, D.ptr(ws), ws.numel(),
                                 D.stream_ptr(dev))
    _lib.check(rc, "sf_potri_diag_batch")


@pytest.mark.parametrize("lda_pad", [0, 16])
@pytest.mark.parametrize("n", [64, 192, 320])
def test_diagonal_of_the_inverse_within_the_componentwise_bound_and_reproducible(gpu, n, lda_pad):
    import torch

    lib, dev = gpu
    lda = n + lda_pad
    kept, L = factors(gpu, n, lda)
    assert lib.sf_potri_diag_workspace_bytes(n, BATCH) >= 8 * BATCH * n * 64
    out_stride = n + 3
    dA = kept.clone()
    out = torch.full((BATCH, out_stride), float("nan"), dtype=torch.float64, device=dev)
    potri_diag(gpu, dA, n, lda, out, out_stride)
    got = out.cpu().numpy()
    assert np.isnan(got[:, n:]).all()  # nothing written behind the n entries
    assert np.isfinite(got[:, :n]).all()
    g2n, gn1 = np.longdouble(2 * gamma(2 * n)), np.longdouble(gamma(n + 1))
    for b in range(BATCH):
        X = inverse_longdouble(L[b])
        aX = np.abs(X)
        d = np.sum(X * X, axis=0)
        bound = g2n * np.sum(aX * (aX @ np.abs(L[b]) @ aX), axis=0) + gn1 * d
        err = np.abs(got[b, :n].astype(np.longdouble) - d)
        worst = float(np.max(err / bound))
        print(f"n={n} lda={lda} matrix {b}: max err / bound = {worst:.3g}, max rel err = {float(np.max(err / d)):.3g}")
        assert (err <= bound).all(), (n, lda, b, worst)
    # the lower triangle was only read
    assert torch.equal(torch.tril(dA[:, :, :n]).cpu(), torch.from_numpy(L.astype(np.float64)))
    # a repeated call, on the upper triangle the first one left: the same bits
    again = torch.full_like(out, float("nan"))
    potri_diag(gpu, dA, n, lda, again, out_stride)
    np.testing.assert_array_equal(again.cpu().numpy(), got)
    # zeros instead of NaN above the diagonal: the same bits
    dZ = kept.clone()
    dZ[:, above_diagonal(n, lda, dev)] = 0.0
    zeros = torch.full_like(out, float("nan"))
    potri_diag(gpu, dZ, n, lda, zeros, out_stride)
    np.testing.assert_array_equal(zeros.cpu().numpy(), got)
    assert torch.equal(torch.tril(dZ[:, :, :n]).cpu(), torch.from_numpy(L.astype(np.float64)))


def test_bad_arguments_are_refused_before_anything_is_enqueued(gpu):
    import torch

    from starfish_amd import _device as D

    lib, dev = gpu
    n, lda = 64, 64
    kept, _ = factors(gpu, n, lda)
    dA = kept.clone()
    before = dA.clone()
    out = torch.full((BATCH, n), float("nan"), dtype=torch.float64, device=dev)
    ws = D.workspace(lib.sf_potri_diag_workspace_bytes(n, BATCH), dev)
    good = dict(L=D.ptr(dA), n=n, lda=lda, stride=n * lda, batch=BATCH, out=D.ptr(out), out_stride=n, work=D.ptr(ws),
                work_bytes=ws.numel())
    bad = [dict(n=0), dict(n=-64), dict(n=96), dict(lda=n - 1), dict(batch=0), dict(out_stride=n - 1), dict(L=None),
           dict(out=None), dict(work=None), dict(work_bytes=ws.numel() - 1), dict(work_bytes=0)]
    for change in bad:
        a = dict(good, **change)
        rc = lib.sf_potri_diag_batch(a["L"], a["n"], a["lda"], a["stride"], a["batch"], a["out"], a["out_stride"], a["work"],
                                     a["work_bytes"], D.stream_ptr(dev))
        assert rc == SF_EINVAL, (change, rc)
        assert lib.sf_last_error().decode().startswith("sf_potri_diag_batch:"), (change, lib.sf_last_error())
    torch.cuda.synchronize(dev)
    assert np.isnan(out.cpu().numpy()).all()
    assert torch.equal(torch.nan_to_num(dA, nan=-1.0), torch.nan_to_num(before, nan=-1.0))
    assert lib.sf_potri_diag_workspace_bytes(0, BATCH) == 0 and lib.sf_potri_diag_workspace_bytes(n, 0) == 0
    assert lib.sf_potri_diag_workspace_bytes(96, BATCH) == 0
