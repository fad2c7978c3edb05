"""The contract of the factor stage (sf_potrf_batch under all five launch sequences, sf_logdet_sqmah_batch) on inputs whose
factor is known exactly (potrf_cases.py): every matrix of the batch against that factor; nothing but the lower triangles read
(NaN above the diagonal, in the row padding, between, before and behind the matrices, in the workspace); nothing outside the
matrices written; pivot failures that an update produces, on the tile edges; the stand-alone solve on given factors, with z
in LDS and in the workspace; every refusal before a launch.  Needs an MI355X: run with -m gpu."""
import ctypes as C

import numpy as np
import pytest

import potrf_cases as PC

pytestmark = pytest.mark.gpu

ATOL = 1e-12           # |L - L0| entrywise: the atol of test_gpu_stages.py for entries of the same size
SF_EINVAL, SF_ENOMEM = -1, -2
SENTINEL = 777
NAN = float("nan")


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from starfish_amd import _lib

    return _lib.require_gpu()


def _sync():
    """Waits for the device; a HIP error ends the session (nothing more is started on a device that has faulted)."""
    import torch

    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"HIP error, session ended: {e}", returncode=3)


# ---- device-side helpers ---------------------------------------------------------------------------------------------------
def _upload(emb):
    from starfish_amd import _device as D

    return D.to_dev(emb.buf, D.device_of())


def _mats(dbuf, emb):
    """(batch, n, n) view of the matrices inside the flat device buffer"""
    import torch

    lay = emb.layout
    return torch.as_strided(dbuf, (emb.batch, lay.n, lay.n), (lay.stride, lay.lda, 1), emb.front)


def _outside_is_nan(dbuf, emb):
    import torch

    probe = dbuf.clone()
    _mats(probe, emb).zero_()
    return int(torch.isnan(probe).sum()) == probe.numel() - emb.batch * emb.layout.n ** 2


def _lower(dbuf, emb):
    import torch

    return torch.tril(_mats(dbuf, emb))


def _same_bits(a, b):
    import torch

    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def _workspace(gpu, n, batch, poison=True):
    import torch
    from starfish_amd import _device as D

    ws = D.workspace(gpu.sf_potrf_workspace_bytes(n, batch), D.device_of())
    if poison:
        ws[: ws.numel() // 8 * 8].view(torch.float64).fill_(NAN)
    return ws


def _potrf(gpu, dbuf, emb, ws):
    """One call on the embedded matrices; returns info (numpy).  The call must succeed."""
    import torch
    from starfish_amd import _device as D, _lib

    lay, dev = emb.layout, D.device_of()
    info = torch.full((emb.batch,), SENTINEL, dtype=torch.int32, device=dev)
    _lib.check(gpu.sf_potrf_batch(C.c_void_p(dbuf.data_ptr() + 8 * emb.front), lay.n, lay.lda, lay.stride, emb.batch, D.ptr(info),
                                  D.ptr(ws), ws.numel(), D.stream_ptr(dev)), "sf_potrf_batch")
    _sync()
    return info.cpu().numpy()


def _layout(n, name):
    return {lay.name: lay for lay in PC.layouts(n)}[name]


def _check_known_factor(gpu, n, batch, layout, tag):
    """Test 1 (+ 3): symmetric upper triangle, fresh workspace; returns the lower triangles (device) for the bit comparisons."""
    L0, A = PC.case(n, batch)
    emb = PC.embed(A, _layout(n, layout))
    dbuf = _upload(emb)
    info = _potrf(gpu, dbuf, emb, _workspace(gpu, n, batch, poison=False))
    assert info.tolist() == [0] * batch
    low = _lower(dbuf, emb)
    err = np.abs(low.cpu().numpy() - L0).reshape(batch, -1).max(axis=1)
    print(f"potrf[{tag}] n={n} batch={batch} {layout}: max |L - L0| = {err.max():.3e} (matrix {int(err.argmax())})")
    assert np.isfinite(err).all() and err.max() <= ATOL, err.tolist()
    assert _outside_is_nan(dbuf, emb), "wrote outside the matrices"
    return low


# ---- 1 + 3: every matrix against the known factor; guards intact -------------------------------------------------------------
@pytest.mark.parametrize("layout", ["tight", "padded"])
@pytest.mark.parametrize("n,batch", PC.SHAPES)
def test_every_matrix_matches_the_known_factor(gpu, chol_sequence, n, batch, layout):
    _check_known_factor(gpu, n, batch, layout, chol_sequence)


@pytest.mark.parametrize("n,batch", PC.SHAPES)
def test_every_matrix_matches_the_known_factor_automatic_choice(gpu, n, batch):
    assert gpu.sf_debug_cholesky_sequence(-1) == 0
    _check_known_factor(gpu, n, batch, "padded", "auto")


# ---- 2 + 3: nothing outside the lower triangles is read, nothing outside the matrices written ----------------------------------
@pytest.mark.parametrize("layout", ["tight", "padded"])
@pytest.mark.parametrize("n,batch", PC.SHAPES)
def test_reads_only_the_lower_triangles(gpu, chol_sequence, n, batch, layout):
    """The lower triangles carry the bits of the clean run (symmetric upper triangle, fresh workspace) when the strict upper
    triangle and the workspace are NaN, and when the workspace is what a call on OTHER matrices of the same shape left."""
    clean = _check_known_factor(gpu, n, batch, layout, chol_sequence)
    _, A = PC.case(n, batch)
    lay = _layout(n, layout)
    ws = _workspace(gpu, n, batch, poison=True)
    emb = PC.embed(A, lay, upper="nan")
    dbuf = _upload(emb)
    assert _potrf(gpu, dbuf, emb, ws).tolist() == [0] * batch
    assert _same_bits(_lower(dbuf, emb), clean), "result depends on the upper triangle or on the workspace's contents"
    assert _outside_is_nan(dbuf, emb), "wrote outside the matrices"
    # the workspace as another batch leaves it
    _, A_other = PC.case(n, batch, seed=1)
    other = PC.embed(A_other, lay, upper="nan")
    dother = _upload(other)
    assert _potrf(gpu, dother, other, ws).tolist() == [0] * batch
    dbuf = _upload(emb)
    assert _potrf(gpu, dbuf, emb, ws).tolist() == [0] * batch
    assert _same_bits(_lower(dbuf, emb), clean), "result depends on what the previous call left in the workspace"
    assert _outside_is_nan(dbuf, emb) and _outside_is_nan(dother, other), "wrote outside the matrices"


# ---- 4: pivot failures that an update produces, on the tile edges ---------------------------------------------------------------
@pytest.mark.parametrize("n,p1,p4", [(n, p1, p4) for n in sorted(PC.PIVOTS) for p1, p4 in PC.pivot_pairs(n)])
def test_pivot_failure_from_an_update(gpu, chol_sequence, n, p1, p4):
    batch = PC.PIVOT_BATCH
    L0, A = PC.case(n, batch)
    lay = _layout(n, "padded")
    emb = PC.embed(A, lay)
    dclean = _upload(emb)
    assert _potrf(gpu, dclean, emb, _workspace(gpu, n, batch)).tolist() == [0] * batch
    clean = _lower(dclean, emb)
    bad = np.array(A)
    bad[1] = PC.not_pd_at(A[1], L0[1], p1)
    bad[4] = PC.not_pd_at(A[4], L0[4], p4)
    embad = PC.embed(bad, lay)
    dbad = _upload(embad)
    info = _potrf(gpu, dbad, embad, _workspace(gpu, n, batch))
    assert info.tolist() == [0, p1 + 1, 0, 0, p4 + 1]
    got = _lower(dbad, embad)
    for b in (0, 2, 3):
        assert _same_bits(got[b], clean[b]), f"matrix {b} differs from the batch without failures"
    for b, p in ((1, p1), (4, p4)):
        assert _same_bits(got[b, :p, :p], clean[b, :p, :p]), f"matrix {b}: the factor left of the failing column {p} is damaged"
    assert _outside_is_nan(dbad, embad), "wrote outside the matrices"


# ---- 5: sf_logdet_sqmah_batch on given factors -----------------------------------------------------------------------------------
def _solve(gpu, Lptr, n, lda, stride, batch, dR, ldr, ws):
    import torch
    from starfish_amd import _device as D

    dev = D.device_of()
    ld = torch.full((batch,), float(SENTINEL), dtype=torch.float64, device=dev)
    sq = torch.full((batch,), float(SENTINEL), dtype=torch.float64, device=dev)
    rc = gpu.sf_logdet_sqmah_batch(C.c_void_p(Lptr), n, lda, stride, batch, D.ptr(dR), ldr, D.ptr(ws), ws.numel() if ws is not None else 0,
                                   D.ptr(ld), D.ptr(sq), D.stream_ptr(dev))
    _sync()
    return rc, ld.cpu().numpy(), sq.cpu().numpy()


@pytest.mark.parametrize("extra_ldr", [0, 2])
@pytest.mark.parametrize("layout", ["tight", "padded"])
@pytest.mark.parametrize("n", [64, 192, 320])
def test_logdet_sqmah_on_given_factors(gpu, n, layout, extra_ldr):
    from starfish_amd import _device as D

    batch = 3
    L0, z0, R, want_ld, want_sq = PC.solve_case(n, batch)
    emb = PC.embed(L0, _layout(n, layout), upper="nan")  # NaN above the diagonal, around and between the factors
    dbuf = _upload(emb)
    before = dbuf.clone()
    ldr = n + extra_ldr
    Rp = np.zeros((batch, ldr))
    Rp[:, :n] = R
    lay = emb.layout
    rc, ld, sq = _solve(gpu, dbuf.data_ptr() + 8 * emb.front, n, lay.lda, lay.stride, batch, D.to_dev(Rp, D.device_of()), ldr,
                        _workspace(gpu, n, batch))
    assert rc == 0
    e_ld, e_sq = np.abs(ld / want_ld - 1).max(), np.abs(sq / want_sq - 1).max()
    print(f"logdet_sqmah n={n} {layout} ldr={ldr}: rel err logdet {e_ld:.3e} sqmah {e_sq:.3e}")
    np.testing.assert_allclose(ld, want_ld, rtol=1e-12)
    np.testing.assert_allclose(sq, want_sq, rtol=1e-11)
    assert _same_bits(dbuf, before), "the solve wrote into the factor's buffer"


def _big_factors(n, batch, seed):
    """On the device: `batch` dyadic factors of order n at lda = n + 16 (off-diagonal non-zeros in a band of half-width 160 and
    in the last 64 rows, so L0 stays well conditioned), NaN above the diagonal and in the padding; R = L0 z0 (exact)."""
    import torch
    from starfish_amd import _device as D

    dev = D.device_of()
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    lda = n + 16
    L = torch.full((batch, n, lda), NAN, dtype=torch.float64, device=dev)
    R = torch.empty((batch, n), dtype=torch.float64, device=dev)
    i = torch.arange(n, device=dev)[:, None]
    j = torch.arange(n, device=dev)[None, :]
    keep = (j < i) & ((i - j <= 160) | (i >= n - 64))
    upper = j > i
    diag, z0 = [], []
    for b in range(batch):
        M = torch.randint(-PC.OFF_RANGE, PC.OFF_RANGE + 1, (n, n), generator=g, device=dev, dtype=torch.float64)
        M = torch.where(keep, M, torch.zeros((), dtype=torch.float64, device=dev)) / PC.Q
        d = torch.randint(PC.Q, 4 * PC.Q + 1, (n,), generator=g, device=dev, dtype=torch.float64) / PC.Q
        M.diagonal().copy_(d)
        z = torch.randint(-PC.Q, PC.Q + 1, (n,), generator=g, device=dev, dtype=torch.float64) / PC.Q
        R[b] = M @ z
        M.masked_fill_(upper, NAN)
        L[b, :, :n] = M
        diag.append(d.cpu().numpy())
        z0.append(z.cpu().numpy())
        del M
    z0 = np.array(z0)
    return L, R, PC.logdet_of(np.array(diag)), (z0 * z0).sum(axis=1)


@pytest.mark.parametrize("n", [16192, 16256])
def test_logdet_sqmah_z_in_lds_and_in_the_workspace(gpu, n):
    """n = 16192 is the last order whose z fits the LDS beside the 64 x 65 block (no workspace needed), 16256 the first that
    keeps z in the workspace: without one the call is refused with SF_ENOMEM before anything is enqueued."""
    from starfish_amd import _device as D

    batch, lda = 2, n + 16
    in_lds = 8 * (64 * 65 + 64 + 8 + n) <= 160 * 1024
    assert in_lds == (n == 16192)
    L, R, want_ld, want_sq = _big_factors(n, batch, seed=n)
    _sync()
    if in_lds:
        ws = None
    else:
        need = gpu.sf_potrf_workspace_bytes(n, batch)
        for short in (None, D.workspace(need, D.device_of())[: need - 1]):
            rc, ld, sq = _solve(gpu, L.data_ptr(), n, lda, n * lda, batch, R, n, short)
            assert rc == SF_ENOMEM
            assert (ld == SENTINEL).all() and (sq == SENTINEL).all()
        ws = _workspace(gpu, n, batch)
    rc, ld, sq = _solve(gpu, L.data_ptr(), n, lda, n * lda, batch, R, n, ws)
    assert rc == 0
    e_ld, e_sq = np.abs(ld / want_ld - 1).max(), np.abs(sq / want_sq - 1).max()
    print(f"logdet_sqmah n={n} z in {'LDS' if in_lds else 'workspace'}: rel err logdet {e_ld:.3e} sqmah {e_sq:.3e}")
    np.testing.assert_allclose(ld, want_ld, rtol=1e-12)
    np.testing.assert_allclose(sq, want_sq, rtol=1e-11)


# ---- 6: argument refusals: no launch, nothing touched ----------------------------------------------------------------------------
def test_argument_refusals_touch_nothing(gpu):
    """Every buffer is large enough for what the refused call names, and holds valid matrices."""
    import torch
    from starfish_amd import _device as D

    dev = D.device_of()
    n, batch = 128, 2
    L0, A = PC.case(n, 3)
    lay = _layout(n, "padded")
    emb = PC.embed(A, lay)  # three matrices: room behind the two the calls name
    dbuf = _upload(emb)
    before = dbuf.clone()
    Aptr = C.c_void_p(dbuf.data_ptr() + 8 * emb.front)
    info = torch.full((batch,), SENTINEL, dtype=torch.int32, device=dev)
    ws = _workspace(gpu, n, batch)
    need = gpu.sf_potrf_workspace_bytes(n, batch)
    assert need > 0 and ws.numel() >= need
    s = D.stream_ptr(dev)
    ok = dict(A=Aptr, n=n, lda=lay.lda, stride=lay.stride, batch=batch, info=D.ptr(info), work=D.ptr(ws), bytes=ws.numel())
    min_stride = (n - 1) * lay.lda + n
    refused = {
        "n = 96": dict(n=96),
        "n = 0": dict(n=0),
        "lda < n": dict(lda=n - 2),
        "lda odd": dict(lda=n + 1),
        "batch = 0": dict(batch=0),
        "batch < 0": dict(batch=-1),
        "null d_A": dict(A=None),
        "null d_info": dict(info=None),
        "null d_work": dict(work=None),
        "workspace one byte short": dict(bytes=need - 1),
        "stride odd": dict(stride=lay.stride + 1),
        "stride overlaps": dict(stride=min_stride - 2),
        "stride = 0": dict(stride=0),
    }
    assert min_stride % 2 == 0  # ("stride overlaps" is refused for its size, not its parity)
    for what, change in refused.items():
        a = dict(ok, **change)
        rc = gpu.sf_potrf_batch(a["A"], a["n"], a["lda"], a["stride"], a["batch"], a["info"], a["work"], a["bytes"], s)
        _sync()
        assert rc == SF_EINVAL, (what, rc)
        assert gpu.sf_last_error(), what
        assert (info == SENTINEL).all(), what
        assert _same_bits(dbuf, before), what
    # the solve
    R = torch.ones((batch, n), dtype=torch.float64, device=dev)
    Lp = dbuf.data_ptr() + 8 * emb.front
    for what, kw in {"ldr < n": dict(ldr=n - 1), "n = 96": dict(n=96), "batch = 0": dict(batch=0), "null d_L": dict(Lptr=None),
                     "null d_R": dict(dR=None)}.items():
        a = dict(dict(Lptr=Lp, n=n, lda=lay.lda, stride=lay.stride, batch=batch, dR=R, ldr=n), **kw)
        rc, ld, sq = _solve(gpu, a["Lptr"], a["n"], a["lda"], a["stride"], a["batch"], a["dR"], a["ldr"], ws)
        assert rc == SF_EINVAL, (what, rc)
        assert (ld == SENTINEL).all() and (sq == SENTINEL).all(), what
    # ... and the same arguments unchanged are accepted
    rc = gpu.sf_potrf_batch(ok["A"], n, lay.lda, lay.stride, batch, ok["info"], ok["work"], ok["bytes"], s)
    _sync()
    assert rc == 0 and info.cpu().tolist() == [0, 0]
    assert np.abs(_lower(dbuf, emb).cpu().numpy()[:batch] - L0[:batch]).max() <= ATOL
