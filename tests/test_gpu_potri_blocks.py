"""sf_potri_blocks_batch alone: selected 64 x 64 blocks of C^-1 = X^T X, X = L^-1, for the L left by a factorisation.

Factors: random well-conditioned matrices through sf_potrf_batch, and the factors the likelihood leaves for the synthetic
orders N = 180, 256, 330 (through DeviceOrder.apply, padded with the identity to 192, 256, 384), everything above the diagonal
-- inside the diagonal blocks too -- NaN: a single read from there before it is written poisons the result.  Pairs: every
(I, I) and (I, I - 1), the corner (nb - 1, 0) and one pair twice.  The reference is G = X^T X with X the np.longdouble inverse of
the very L the device reads.  Bound, entrywise, with u = 2^-53 and gamma_k = k u / (1 - k u):
    |G^ - G| <= gamma_2n (E + E^T) + gamma_{n+1} |X|^T |X|,   E = |X|^T |X||L||X|
(tests/test_gpu_potri_diag.py: |dX| <= gamma_2n |X||L||X| to first order, G = X^T X turns it into |dX|^T |X| + |X|^T |dX|, and the
second term is the product itself).  The bound's own matrix products are evaluated in float64."""
import numpy as np
import pytest

from starfish_amd import synth

from gpu_helpers import device_order, oracle_order, pack_rows

pytestmark = pytest.mark.gpu

BATCH = 3
U = 2.0 ** -53
ORDER_OF = {192: 180, 256: 256, 384: 330}


def gamma(k):
    return k * U / (1 - k * U)


@pytest.fixture(scope="module")
def gpu():
    import torch

    from starfish_amd import _lib

    lib = _lib.require_gpu()
    return lib, torch.device("cuda", torch.cuda.current_device())


def inverse_longdouble(L):
    """X = L^-1 by forward substitution, row by row, in the precision of L (as tests/test_gpu_pointwise.py)."""
    X = np.zeros_like(L)
    for i in range(L.shape[0]):
        row = -(L[i, :i] @ X[:i])
        row[i] += 1
        X[i] = row / L[i, i]
    return X


def random_factors(gpu, n):
    import torch

    from starfish_amd import _device as D, _lib

    lib, dev = gpu
    rng = np.random.default_rng(7000 + n)
    A = np.zeros((BATCH, n, n))
    for b in range(BATCH):
        G = rng.standard_normal((n, n))
        A[b] = G @ G.T + n * np.eye(n)
    dA = D.to_dev(A, dev)
    info = torch.zeros(BATCH, dtype=torch.int32, device=dev)
    ws = D.workspace(lib.sf_potrf_workspace_bytes(n, BATCH), dev)
    _lib.check(lib.sf_potrf_batch(D.ptr(dA), n, n, n * n, BATCH, D.ptr(info), D.ptr(ws), ws.numel(), D.stream_ptr(dev)),
               "sf_potrf_batch")
    torch.cuda.synchronize(dev)
    assert (info.cpu().numpy() == 0).all()
    return np.tril(dA.cpu().numpy())


def order_factors(n):
    """The factors of the three walkers of the synthetic order whose padded size is n, identity on the padding."""
    N = ORDER_OF[n]
    o = synth.make_order(N=N, m=4, seed=5)
    do = device_order(oracle_order(o))
    assert do.npad == n
    md, rows = pack_rows(do, [synth.vector_to_oracle_params(p) for p in synth.walker_ball(o, B=BATCH, seed=3)])
    out = do.apply(md, rows, "L", rhs=np.eye(N))  # L e_j sums one product by 1 and zeros: the factor, exactly
    assert (out["info"] == 0).all()
    L = np.tile(np.eye(n), (BATCH, 1, 1))
    L[:, :N, :N] = np.tril(np.transpose(out["out"], (0, 2, 1)))
    return L


_CASES = {}


def case(gpu, kind, n):
    """(L (BATCH, n, n) float64 lower triangular, reference G (BATCH, n, n) longdouble, bound (BATCH, n, n)); made once."""
    if (kind, n) not in _CASES:
        L = random_factors(gpu, n) if kind == "random" else order_factors(n)
        assert np.isfinite(L).all()
        G, bound = [], []
        for b in range(BATCH):
            X = inverse_longdouble(L[b].astype(np.longdouble))
            G.append(X.T @ X)
            aX, aL = np.abs(X).astype(np.float64), np.abs(L[b])
            E = aX.T @ (aX @ (aL @ aX))
            bound.append(gamma(2 * n) * (E + E.T) + gamma(n + 1) * (aX.T @ aX))
        _CASES[(kind, n)] = (L, np.stack(G), np.stack(bound))
    return _CASES[(kind, n)]


def pairs_of(nb):
    pairs = [(I, I) for I in range(nb)] + [(I, I - 1) for I in range(1, nb)] + [(nb - 1, 0), (1, 0)]
    assert pairs.count((1, 0)) == 2  # one pair twice
    return np.array(pairs, dtype=np.int32)


def potri_blocks(gpu, dA, n, lda, d_pairs, npairs, out):
    from starfish_amd import _device as D, _lib

    lib, dev = gpu
    ws = D.workspace(lib.sf_potri_blocks_workspace_bytes(n, BATCH), dev)
    rc = lib.sf_potri_blocks_batch(D.ptr(dA), n, lda, n * lda, BATCH, D.ptr(d_pairs), npairs, D.ptr(out), D.ptr(ws), ws.numel(),
                                   D.stream_ptr(dev))
    _lib.check(rc, "sf_potri_blocks_batch")


@pytest.mark.parametrize("kind", ["random", "order"])
@pytest.mark.parametrize("n", [192, 256, 384])
def test_blocks_of_the_inverse_within_the_entrywise_bound_and_reproducible(gpu, n, kind):
    import torch

    lib, dev = gpu
    L, G, bound = case(gpu, kind, n)
    lda = n + 16
    host = np.full((BATCH, n, lda), np.nan)
    rows, cols = np.tril_indices(n)
    host[:, rows, cols] = L[:, rows, cols]
    dA = torch.from_numpy(host).to(dev)
    nb = n // 64
    pairs = pairs_of(nb)
    d_pairs = torch.from_numpy(pairs).to(dev)
    out = torch.full((BATCH, len(pairs), 64, 64), float("nan"), dtype=torch.float64, device=dev)
    potri_blocks(gpu, dA, n, lda, d_pairs, len(pairs), out)
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    worst = 0.0
    for b in range(BATCH):
        for k, (I, J) in enumerate(pairs):
            blk = np.s_[64 * I:64 * I + 64, 64 * J:64 * J + 64]
            err = np.abs(got[b, k].astype(np.longdouble) - G[b][blk])
            pos = bound[b][blk] > 0  # (exact zeros between the identity padding and the data: bound 0, error 0)
            ratio = float((err[pos] / bound[b][blk][pos]).max())
            worst = max(worst, ratio)
            assert (err <= bound[b][blk]).all(), (kind, n, b, int(I), int(J), ratio)
    print(f"{kind} n={n}: {len(pairs)} pairs x {BATCH} matrices: max err / bound = {worst:.3g}")
    np.testing.assert_array_equal(got[:, -1], got[:, nb])  # the pair listed twice: (1, 0) is also pairs[nb]
    assert tuple(pairs[nb]) == (1, 0)
    # the lower triangle and the whole diagonal blocks (their NaN above the diagonal too) are as they were
    after = dA.cpu().numpy()
    np.testing.assert_array_equal(after[:, rows, cols], L[:, rows, cols])
    for I in range(nb):
        blk = np.s_[:, 64 * I:64 * I + 64, 64 * I:64 * I + 64]
        np.testing.assert_array_equal(np.nan_to_num(after[blk], nan=-1.0), np.nan_to_num(host[blk], nan=-1.0))
    assert np.isnan(after[:, :, n:]).all()  # nothing written behind the n columns
    # a repeated call, on the upper triangle the first one left: the same bits
    again = torch.full_like(out, float("nan"))
    potri_blocks(gpu, dA, n, lda, d_pairs, len(pairs), again)
    np.testing.assert_array_equal(again.cpu().numpy(), got)


def test_a_pair_outside_the_matrix_gives_nan_and_the_others_their_bits(gpu):
    import torch

    lib, dev = gpu
    n = 192
    L, _, _ = case(gpu, "random", n)
    dA = torch.from_numpy(np.ascontiguousarray(L)).to(dev)
    pairs = np.array([(2, 1), (0, 1), (3, 0), (1, -1), (2, 2)], dtype=np.int32)
    d_pairs = torch.from_numpy(pairs).to(dev)
    out = torch.full((BATCH, len(pairs), 64, 64), 7.0, dtype=torch.float64, device=dev)
    potri_blocks(gpu, dA, n, n, d_pairs, len(pairs), out)
    got = out.cpu().numpy()
    assert np.isnan(got[:, 1:4]).all() and np.isfinite(got[:, [0, 4]]).all()
    good = torch.full((BATCH, 2, 64, 64), 7.0, dtype=torch.float64, device=dev)
    potri_blocks(gpu, dA, n, n, torch.from_numpy(pairs[[0, 4]].copy()).to(dev), 2, good)
    np.testing.assert_array_equal(good.cpu().numpy(), got[:, [0, 4]])
