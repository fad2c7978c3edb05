"""Emulator.train(batch_simplex=True): the host side, without a GPU.  The C-ABI table of the batched training objective, and
the filter / raiser / fall-back logic of the batched objective with a stand-in for the device evaluator (a numpy function
of the rows: Emulator.log_likelihood_batch and Emulator.log_likelihood replaced on the instance)."""
import os
import re
import warnings

import numpy as np
import pytest
from scipy.linalg import cho_factor, cho_solve
from scipy.optimize import minimize

from starfish_amd import _lib, synth
from starfish_amd._neldermead import minimize_neldermead_batched
from starfish_amd.emulator import Emulator
from starfish_amd.emulator.kernels import batch_kernel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sf_emulator_v11_build_batch", "sf_emulator_loglike_workspace_bytes", "sf_emulator_loglike_batch")


def test_the_new_entry_points_are_declared_and_bound_with_matching_argument_counts():
    header = open(os.path.join(ROOT, "include", "starfish_amd.h")).read()
    for name in NEW:
        found = re.findall(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", header)
        assert len(found) == 1, f"{name} is not declared (once) in include/starfish_amd.h"
        nargs = len([a for a in found[0].split(",") if a.strip() and a.strip() != "void"])
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert len(_lib.SIGNATURES[name][1]) == nargs, name


def _emulator(m=2, seed=3):
    o = synth.make_order(N=256, m=m, seed=seed)
    return Emulator(o["grid_points"], o["param_names"], o["emu_wl"], o["weights"], o["eigenspectra"], o["w_hat"],
                    o["flux_mean"], o["flux_std"], o["factors"])


def _host_loglike(emu, row):
    """The reference's algorithm for one hyper-parameter vector (emulator.py:602-619), numpy + LAPACK."""
    m = emu.ncomps
    lam, var, ls = np.exp(row[0]), np.exp(row[1:1 + m]), np.exp(row[1 + m:]).reshape(m, -1)
    v11 = emu.iPhiPhi / lam + batch_kernel(emu.grid_points, emu.grid_points, var, ls)
    f = cho_factor(v11)
    return -(2 * np.sum(np.log(f[0].diagonal())) + emu.w_hat @ cho_solve(f, emu.w_hat)) / 2


def _host_batch(emu):
    def evaluate(X, return_info=True):
        assert return_info
        return np.array([_host_loglike(emu, r) for r in X]), np.zeros(len(X), dtype=np.int32)

    return evaluate


def test_rows_the_scalar_objective_rejects_never_reach_the_evaluator():
    emu = _emulator()
    P0 = emu.get_param_vector()
    keys = list(emu.get_param_dict())
    seen = []

    def evaluate(X):
        seen.append(np.array(X))
        return -np.sum(X * X, axis=1), np.zeros(len(X), dtype=np.int32)

    X = np.tile(P0, (5, 1))
    X[1, 2] = np.nan
    X[2, 0] = np.inf
    short = keys.index("log_lengthscale:1:0")
    X[3, short] = np.log(1.9 * emu._grid_sep[0])  # below twice the grid separation of that axis
    X[4, 1] += 0.25
    vals, raiser = emu._batched_objective(evaluate)(X)
    assert len(seen) == 1
    np.testing.assert_array_equal(seen[0], X[[0, 4]])
    np.testing.assert_array_equal(vals[[1, 2, 3]], [np.inf] * 3)
    np.testing.assert_array_equal(vals[[0, 4]], np.sum(X[[0, 4]] ** 2, axis=1))
    for i in range(5):
        raiser(i)  # no row failed on the device: nothing raises
    np.testing.assert_array_equal(emu.get_param_vector(), P0)
    # a batch without a single admissible row makes no call at all
    vals, _ = emu._batched_objective(evaluate)(X[1:4])
    assert len(seen) == 1 and np.isinf(vals).all()


def test_a_failed_row_raises_only_when_the_method_uses_its_value():
    emu = _emulator()
    P0 = emu.get_param_vector()

    def failing(bad_rows):
        def evaluate(X):
            lnl = -np.sum((X - P0) ** 2, axis=1)
            info = np.zeros(len(X), dtype=np.int32)
            if len(X) == 4:  # the candidates of an iteration: reflection, expansion, outside and inside contraction
                info[bad_rows] = 7
                lnl[bad_rows] = -np.inf
            return lnl, info

        return evaluate

    x0 = P0 + 0.3
    # P0 is the minimum: from x0 the reflection never beats the best vertex in the first iterations, so the expansion
    # (row 1) is a discarded speculative point: its failure is silent and the run equals the one without it
    clean = minimize_neldermead_batched(emu._batched_objective(failing([])), x0, maxiter=3)
    quiet = minimize_neldermead_batched(emu._batched_objective(failing([1])), x0, maxiter=3)
    assert (quiet.nit, quiet.nfev) == (clean.nit, clean.nfev) and quiet.nfev < quiet.nfev_speculative
    np.testing.assert_array_equal(quiet.x, clean.x)
    # the reflection (row 0) is used by every iteration: the scalar path's error, with its message
    with pytest.raises(np.linalg.LinAlgError, match="7-th leading minor of the array is not positive definite"):
        minimize_neldermead_batched(emu._batched_objective(failing([0])), x0, maxiter=3)


def test_batched_train_over_a_host_evaluator_is_scipys_run_bit_for_bit():
    opts = dict(maxiter=25)
    ref = _emulator()

    def nll(P):  # Emulator.train's scalar objective over the host likelihood
        if np.any(~np.isfinite(P)):
            return np.inf
        if np.any(np.exp(P[1 + ref.ncomps:]).reshape(ref.ncomps, -1) < 2 * ref._grid_sep):
            return np.inf
        return -_host_loglike(ref, P)

    want = minimize(nll, ref.get_param_vector(), method="Nelder-Mead", options=opts)
    emu = _emulator()
    emu.log_likelihood_batch = _host_batch(emu)
    got = emu.train(batch_simplex=True, options=opts)
    assert (got.nit, got.nfev, got.status) == (want.nit, want.nfev, want.status)
    np.testing.assert_array_equal(got.x, want.x)
    assert got.fun == want.fun
    assert got.nbatches <= got.nit + 2 and got.nfev_speculative >= got.nfev
    # maxiter ends the run: not a success, the emulator stands at the last point the objective was asked for
    assert not got.success and emu._trained is False
    np.testing.assert_array_equal(emu.get_param_vector(), got.last_x)


def test_unsupported_arguments_fall_back_to_the_serial_loop_with_a_warning():
    emu = _emulator()
    calls = []

    def scalar():
        calls.append(1)
        return _host_loglike(emu, emu.get_param_vector())

    def never(X, return_info=False):
        raise AssertionError("the batched evaluator must not run on the serial path")

    emu.log_likelihood = scalar
    emu.log_likelihood_batch = never
    with pytest.warns(RuntimeWarning, match="Powell"):
        soln = emu.train(batch_simplex=True, method="Powell", options=dict(maxiter=1, maxfev=20))
    assert calls and not hasattr(soln, "nbatches")
    # the default is the serial loop, silently
    calls.clear()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        soln = emu.train(options=dict(maxiter=3))
    assert calls and not hasattr(soln, "nbatches")


def test_argument_checks_come_before_anything_is_enqueued():
    """No GPU: the refused calls return from the host-side checks (the pointers are dummies that nothing dereferences)."""
    lib = _lib.load()
    M, m, B = 27, 2, 3
    npad, lda = 64, 80
    need = lib.sf_emulator_loglike_workspace_bytes(M, m, B)
    # the B matrices, the B x npad right-hand sides and the factorisation's workspace, plus logdet / sqmah / info
    assert need >= 8 * B * npad * lda + 8 * B * npad + lib.sf_potrf_workspace_bytes(npad, B)
    assert need <= 8 * B * npad * lda + 8 * B * npad + lib.sf_potrf_workspace_bytes(npad, B) + 5 * 256
    assert lib.sf_emulator_loglike_workspace_bytes(M, m, B + 1) > need
    assert lib.sf_emulator_loglike_workspace_bytes(0, m, B) == 0 and lib.sf_emulator_loglike_workspace_bytes(M, m, 0) == 0
    p = 4096  # a dummy, 256-byte aligned "device pointer"
    EINVAL, ENOMEM = -1, -2

    def loglike(P=3, hyper_stride=9, work=p, work_bytes=need, lnl=p):
        return lib.sf_emulator_loglike_batch(p, M, P, m, p, hyper_stride, B, p, p, lnl, None, None, p, work, work_bytes, None)

    assert loglike(work_bytes=need - 1) == ENOMEM
    assert b"workspace" in lib.sf_last_error()
    assert loglike(P=9, hyper_stride=21) == EINVAL  # more grid dimensions than the build kernel's LDS holds
    assert b"P=9" in lib.sf_last_error()
    assert loglike(hyper_stride=8) == EINVAL
    assert loglike(lnl=None) == EINVAL
    assert loglike(work=None) == EINVAL
    assert loglike(work=p + 8) == EINVAL

    def build(P=3, hyper_stride=9, npad=npad, lda=lda, stride=npad * lda, A=p, R=None, w_hat=None, ldr=0):
        return lib.sf_emulator_v11_build_batch(p, M, P, m, p, hyper_stride, B, p, A, npad, lda, stride, 0, w_hat, R, ldr, None)

    assert build(P=9, hyper_stride=21) == EINVAL
    assert build(lda=81, stride=64 * 81 + 1) == EINVAL      # odd row stride: the 16-byte stores
    assert build(stride=npad * lda + 1) == EINVAL
    assert build(A=p + 8) == EINVAL
    assert build(npad=54, lda=80) == EINVAL                 # not a multiple of the tile
    assert build(npad=0, lda=80) == EINVAL
    assert build(hyper_stride=8) == EINVAL
    assert build(R=p, w_hat=p, ldr=npad - 1) == EINVAL
    assert build(R=p, w_hat=None, ldr=npad) == EINVAL
