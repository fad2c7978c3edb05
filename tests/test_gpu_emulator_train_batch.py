"""Emulator.train with the simplex evaluated in batches on the GPU: the batched build of v11 (k_v11_build_batch), the
training objective for B hyper-parameter vectors in one enqueue (sf_emulator_loglike_batch), Emulator.log_likelihood_batch
and Emulator.train(batch_simplex=True) against the serial scipy loop.  Small matrices, chosen for where the build and the
factorisation behind it take another path (see SHAPES).  Run with -m gpu.  (tests/test_emulator_train_batch_host.py holds
the host logic on the CPU.)"""
import time

import numpy as np
import pytest
from scipy.linalg import cho_factor, cho_solve

from conftest import load_golden
from starfish_amd import synth
from starfish_amd.emulator import Emulator
from starfish_amd.emulator.kernels import batch_kernel

pytestmark = pytest.mark.gpu

AXES16 = ((6000.0, 6100.0, 6200.0, 6300.0), (4.0, 4.5), (-1.0, -0.5))  # a 4 x 2 x 2 library: M = 16
# (m, grid_axes): n = m M and what it exercises
SHAPES = {
    "m4_M16": (4, AXES16),  # n = 64 = npad: no identity padding at all, one tile
    "m2_M27": (2, None),    # n = 54, npad 64: padding and a component boundary inside the only tile
    "m5_M27": (5, None),    # n = 135, npad 192: 64 mod 128 rows (shifted frame), straddling and off-component tiles
    "m8_M27": (8, None),    # n = 216, npad 256: two full 128-panels (golden values: emulator.npz, tag a)
}
SF_EINVAL = -1


def _emulator(m, grid_axes=None, seed=3, **kw):
    o = synth.make_order(N=256, m=m, seed=seed, grid_axes=grid_axes)
    return Emulator(o["grid_points"], o["param_names"], o["emu_wl"], o["weights"], o["eigenspectra"], o["w_hat"],
                    o["flux_mean"], o["flux_std"], o["factors"], **kw)


def _host_loglike(emu, row):
    """numpy v11 + scipy cho_factor / cho_solve: the reference's algorithm (emulator.py:602-619) for one row of logs."""
    m = emu.ncomps
    lam, var, ls = np.exp(row[0]), np.exp(row[1:1 + m]), np.exp(row[1 + m:]).reshape(m, -1)
    v11 = emu.iPhiPhi / lam + batch_kernel(emu.grid_points, emu.grid_points, var, ls)
    f = cho_factor(v11)
    return -(2 * np.sum(np.log(f[0].diagonal())) + emu.w_hat @ cho_solve(f, emu.w_hat)) / 2


def _build(emu, hyper, lower_only, P=None, pad=(34, 3, 8)):
    """sf_emulator_v11_build_batch into NaN-filled arrays with slack between the matrices, after the hyper-parameter
    rows and after the right-hand sides -> (rc, A [B][stride], R [B][ldr], npad, lda)."""
    import torch

    from starfish_amd import _device as D
    from starfish_amd import _lib

    lib = _lib.require_gpu()
    dev = D.device_of()
    M, npar = emu.grid_points.shape
    m = emu.ncomps
    n = m * M
    npad = -(-n // 64) * 64
    lda = npad + 16
    stride, ldr = npad * lda + pad[0], npad + pad[2]
    B = len(hyper)
    rows = np.full((B, hyper.shape[1] + pad[1]), np.nan)
    rows[:, :hyper.shape[1]] = hyper
    A = torch.full((B, stride), np.nan, dtype=torch.float64, device=dev)
    R = torch.full((B, ldr), np.nan, dtype=torch.float64, device=dev)
    d_rows, d_grid = D.to_dev(rows, dev), D.to_dev(emu.grid_points, dev)
    d_iphiphi, d_w = D.to_dev(emu.iPhiPhi, dev), D.to_dev(emu.w_hat, dev)
    rc = lib.sf_emulator_v11_build_batch(D.ptr(d_grid), M, npar if P is None else P, m, D.ptr(d_rows), rows.shape[1], B,
                                         D.ptr(d_iphiphi), D.ptr(A), npad, lda, stride, lower_only, D.ptr(d_w), D.ptr(R), ldr,
                                         D.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    return rc, A.cpu().numpy(), R.cpu().numpy(), npad, lda


@pytest.mark.parametrize("shape", list(SHAPES))
def test_batched_build_matches_the_host_matrix_and_touches_nothing_else(shape):
    m, axes = SHAPES[shape]
    emu = _emulator(m, axes)
    n = m * len(emu.grid_points)
    rng = np.random.default_rng(11)
    B = 3
    lam = np.array([1.7, 0.6, 3.1])
    var = np.exp(rng.uniform(2, 8, (B, m)))
    ls = np.exp(rng.uniform(-0.5, 0.5, (B, m, 3))) * np.array([300.0, 1.5, 1.5])
    hyper = np.concatenate([lam[:, None], var, ls.reshape(B, -1)], axis=1)
    rc, A, R, npad, lda = _build(emu, hyper, 0)
    assert rc == 0
    full = A[:, :npad * lda].reshape(B, npad, lda)
    for b in range(B):
        want = emu.iPhiPhi / lam[b] + batch_kernel(emu.grid_points, emu.grid_points, var[b], ls[b])
        np.testing.assert_allclose(full[b, :n, :n], want, rtol=1e-13, atol=1e-300)
        np.testing.assert_array_equal(full[b, n:, :npad], np.eye(npad)[n:])  # the identity block, exactly
        assert not full[b, :n, n:npad].any()
    assert np.isnan(full[:, :, npad:]).all()      # columns npad..lda of every row
    assert np.isnan(A[:, npad * lda:]).all()      # the gap between matrices
    np.testing.assert_array_equal(R[:, :n], np.tile(emu.w_hat, (B, 1)))
    assert not R[:, n:npad].any() and np.isnan(R[:, npad:]).all()
    # the lower triangles alone: the same bits; tiles strictly above the diagonal are not written at all
    rc, A1, R1, _, _ = _build(emu, hyper, 1)
    assert rc == 0
    low = A1[:, :npad * lda].reshape(B, npad, lda)
    il, jl = np.tril_indices(npad)
    np.testing.assert_array_equal(low[:, il, jl], full[:, il, jl])
    np.testing.assert_array_equal(R1, R)
    if npad > 64:
        assert np.isnan(low[:, :64, 64:]).all()
    # no dependence on the position in the batch: every row built alone
    for b in range(B):
        rc, Ab, Rb, _, _ = _build(emu, hyper[b:b + 1], 0)
        assert rc == 0
        np.testing.assert_array_equal(Ab[0], A[b])
        np.testing.assert_array_equal(Rb[0], R[b])


def test_batched_build_refuses_more_grid_dimensions_than_its_lds_holds():
    emu = _emulator(2)
    hyper = np.ones((2, 1 + 2 + 2 * 9))
    rc, A, R, _, _ = _build(emu, hyper, 0, P=9)
    assert rc == SF_EINVAL
    assert np.isnan(A).all() and np.isnan(R).all()


@pytest.mark.parametrize("tag,m", [("a", 8), ("b", 4)])
def test_batched_likelihood_vs_reference(tag, m):
    g = load_golden("emulator.npz")
    emu = _emulator(m, variances=g[f"{tag}_variances"], lengthscales=g[f"{tag}_lengthscales"])
    P0 = g[f"{tag}_train_P0"]
    np.testing.assert_allclose(emu.get_param_vector(), P0, rtol=1e-14)
    before = emu.get_param_vector()
    got, info = emu.log_likelihood_batch(np.stack([P0, P0 + 0.05]), return_info=True)
    want = np.array([g[f"{tag}_loglike"][0], g[f"{tag}_loglike_shifted"][0]])
    print(f"tag {tag}: rel err vs reference {np.abs(got - want) / np.abs(want)}")
    assert (info == 0).all()
    assert np.all(np.abs(got - want) <= 1e-9 * np.abs(want)), (got, want)
    np.testing.assert_array_equal(emu.get_param_vector(), before)


@pytest.mark.parametrize("shape", ["m4_M16", "m5_M27"])
def test_batched_likelihood_vs_scalar_path_and_host_algorithm(shape):
    m, axes = SHAPES[shape]
    emu = _emulator(m, axes)
    P0 = emu.get_param_vector()
    rng = np.random.default_rng(5)
    P = np.vstack([P0, P0 + rng.choice([-0.1, 0.1], size=(4, P0.size))])
    got = emu.log_likelihood_batch(P)
    assert got.shape == (5,) and emu._trained is False
    np.testing.assert_array_equal(emu.get_param_vector(), P0)
    host = np.array([_host_loglike(emu, r) for r in P])
    print(f"{shape}: rel err vs numpy + scipy {np.abs(got - host) / np.abs(host)}")
    assert np.all(np.abs(got - host) <= 1e-9 * np.abs(host)), (got, host)
    # deterministic, also over a workspace that holds NaN everywhere (the tiles above the diagonal, which the lower-only
    # build leaves out, are never read)
    np.testing.assert_array_equal(emu.log_likelihood_batch(P), got)
    emu._train_dev["ws_batch"].fill_(255)
    np.testing.assert_array_equal(emu.log_likelihood_batch(P), got)
    one = emu.log_likelihood_batch(P[3])  # B = 1
    assert one.shape == (1,) and abs(one[0] - got[3]) <= 1e-12 * abs(got[3])
    scalar = []
    for r in P:
        emu.set_param_vector(r)
        scalar.append(emu.log_likelihood())
    scalar = np.array(scalar)
    print(f"{shape}: rel diff batch vs scalar path {np.abs(got - scalar) / np.abs(scalar)}")
    assert np.all(np.abs(got - scalar) <= 1e-12 * np.abs(scalar)), (got, scalar)
    # a matrix assigned by hand has no hyper-parameter row
    emu.v11 = emu.v11 + 0.5 * np.eye(len(emu.v11))
    with pytest.raises(ValueError, match="assigned by hand"):
        emu.log_likelihood_batch(P)


def test_an_indefinite_row_is_reported_and_leaves_the_other_rows_alone():
    import torch

    from starfish_amd import _device as D
    from starfish_amd import _lib

    lib = _lib.require_gpu()
    dev = D.device_of()
    emu = _emulator(2)
    M, npar = emu.grid_points.shape
    m = 2
    good = np.array([np.concatenate([[lam], emu.variances * s, emu.lengthscales.ravel() * s])
                     for lam, s in ((1.0, 1.0), (1.3, 0.9), (0.8, 1.1))])
    bad = np.concatenate([[-1.0], np.full(m, 1e-6), emu.lengthscales.ravel()])  # -iPhiPhi + 1e-6 RBF: indefinite
    d_grid, d_iphiphi, d_w = D.to_dev(emu.grid_points, dev), D.to_dev(emu.iPhiPhi, dev), D.to_dev(emu.w_hat, dev)

    def run(rows):
        B = len(rows)
        need = lib.sf_emulator_loglike_workspace_bytes(M, m, B)
        assert need > 0
        ws = D.workspace(need, dev)
        d_rows = D.to_dev(rows, dev)
        out = torch.full((3, B), np.nan, dtype=torch.float64, device=dev)
        info = torch.full((B,), 99, dtype=torch.int32, device=dev)
        args = (D.ptr(d_grid), M, npar, m, D.ptr(d_rows), rows.shape[1], B, D.ptr(d_iphiphi), D.ptr(d_w), D.ptr(out[0]),
                D.ptr(out[1]), D.ptr(out[2]), D.ptr(info), D.ptr(ws))
        assert lib.sf_emulator_loglike_batch(*args, need - 1, D.stream_ptr(dev)) == -2  # SF_ENOMEM: nothing enqueued
        _lib.check(lib.sf_emulator_loglike_batch(*args, ws.numel(), D.stream_ptr(dev)), "sf_emulator_loglike_batch")
        return out.cpu().numpy(), info.cpu().numpy()

    clean, info0 = run(good)
    assert (info0 == 0).all() and np.isfinite(clean).all()
    np.testing.assert_allclose(clean[0], -(clean[1] + clean[2]) / 2, rtol=1e-15)
    mixed, info1 = run(np.vstack([good[:2], bad, good[2:]]))
    assert info1[2] > 0 and mixed[0, 2] == -np.inf
    assert not np.isnan(mixed[0]).any()
    assert (info1[[0, 1, 3]] == 0).all()
    np.testing.assert_allclose(mixed[0, [0, 1, 3]], clean[0], rtol=1e-12)


def _pair(m=2, seed=3):
    return _emulator(m, seed=seed), _emulator(m, seed=seed)


def test_batched_train_follows_the_serial_loops_iterates():
    """m = 2, M = 27 (7 hyper-parameters), seed 3: the assertions and tolerances of tests/test_gpu_train.py, for the same
    reason -- the function values of a batch differ from those of a batch of one in the last bits.  Seed 3 (the seed of the
    golden emulator cases) has NOT been checked on an MI355X yet: if a near tie orders differently within these 40
    iterations, another seed is to be chosen and named here, the comparison stays."""
    opts = dict(maxiter=40, return_all=True)
    a, b = _pair()
    want = a.train(options=opts)
    got = b.train(batch_simplex=True, options=opts)
    assert (got.nit, got.nfev, got.status) == (want.nit, want.nfev, want.status)
    assert len(got.allvecs) == len(want.allvecs)
    for x, y in zip(got.allvecs, want.allvecs):
        np.testing.assert_allclose(x, y, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(got.final_simplex[1], want.final_simplex[1], rtol=1e-10)
    assert got.nbatches <= got.nit + 2 and got.nfev_speculative >= got.nfev
    np.testing.assert_allclose(b.get_param_vector(), a.get_param_vector(), rtol=1e-9)
    assert a._trained == b._trained


def test_a_converging_batched_run_trains_the_emulator():
    emu = _emulator(2)
    soln = emu.train(batch_simplex=True, options=dict(xatol=1e-2, fatol=1e-2, maxiter=2000))
    print(f"converging run: nit {soln.nit}, nfev {soln.nfev}, {soln.nbatches} device calls, {soln.nfev_speculative} rows")
    assert soln.success and emu._trained is True
    np.testing.assert_array_equal(emu.get_param_vector(), soln.x)


def test_batched_simplex_is_faster_than_the_serial_loop_at_the_worked_example_size():
    """m = 4, M = 330 (a 1320 x 1320 matrix, 17 hyper-parameters): the same 12 iterations, serial then batched, after one
    warm-up call of each path.  The yardstick is the serial loop measured in the same process.  The ratio has not been
    measured yet (the test prints it)."""
    o = synth.make_order(N=256, m=4, seed=13, grid_axes=synth.BIG_GRID_AXES)
    a, b = (Emulator(o["grid_points"], o["param_names"], o["emu_wl"], o["weights"], o["eigenspectra"], o["w_hat"],
                     o["flux_mean"], o["flux_std"], o["factors"]) for _ in range(2))
    for e in (a, b):
        e.log_likelihood()
        e.log_likelihood_batch(np.tile(e.get_param_vector(), (18, 1)))
    opts = dict(maxiter=12)
    t0 = time.perf_counter()
    s1 = a.train(options=opts)
    t_serial = time.perf_counter() - t0
    t0 = time.perf_counter()
    s2 = b.train(batch_simplex=True, options=opts)
    t_batched = time.perf_counter() - t0
    print(f"Emulator.train, m M = 1320, 12 iterations ({s1.nfev} evaluations): serial {t_serial * 1e3:.1f} ms, batched "
          f"{t_batched * 1e3:.1f} ms ({s2.nbatches} device calls, {s2.nfev_speculative} rows): ratio {t_serial / t_batched:.2f}")
    assert s1.nit == s2.nit == 12 and s1.nfev == s2.nfev
    assert t_batched < t_serial
