"""The emulator training likelihood's gradient without a device: (a) the numpy helper of the GPU test
(tests/emulator_derivatives.py) against the package's host matrix and against a 5-point stencil of its own values in
longdouble, (b) the identity d lnL / d theta = 1/2 sum (alpha alpha^T - V^-1) o dV/dtheta (Rasmussen & Williams, GPML,
eq. 5.9) against a 5-point stencil of the host likelihood in longdouble at the four shapes of the GPU test, with the
n - tr(G K) form of the lambda_xi slot as a cross-check, (c) the refusals of sf_emulator_loglike_grad_batch that need no
device, and (d) Emulator.train(gradient=True) over a stand-in evaluator."""
import os
import re

import numpy as np
import pytest
from scipy.optimize import Bounds

from starfish_amd import _lib, synth
from starfish_amd.emulator import Emulator
from starfish_amd.emulator.kernels import batch_kernel

import emulator_derivatives as ED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
AXES16 = ((6000.0, 6100.0, 6200.0, 6300.0), (4.0, 4.5), (-1.0, -0.5))
AXES2 = ((6000.0, 6100.0, 6200.0, 6300.0, 6400.0), (4.0, 4.5, 5.0))  # two grid axes: M = 15, P = 2
SHAPES = {"m4_M16": (4, AXES16), "m2_M27": (2, None), "m5_M27": (5, None), "m8_M27": (8, None)}
SF_EINVAL, SF_ENOMEM = -1, -2


def _emulator(m=2, grid_axes=None, seed=3):
    o = synth.make_order(N=256, m=m, seed=seed, grid_axes=grid_axes)
    return Emulator(o["grid_points"], o["param_names"], o["emu_wl"], o["weights"], o["eigenspectra"], o["w_hat"],
                    o["flux_mean"], o["flux_std"], o["factors"])


def stencil(f, x, h):
    """5-point first derivative: truncation h^4 / 30 |f^(5)|."""
    return (-f(x + 2 * h) + 8 * f(x + h) - 8 * f(x - h) + f(x - 2 * h)) / (12 * h)


def displaced_row(emu, seed=7):
    """The defaults moved by up to 0.3 in every log: distinct lengthscales per component and axis."""
    rng = np.random.default_rng(seed)
    P0 = emu.get_param_vector()
    return P0 + rng.uniform(-0.3, 0.3, P0.size)


# ------------------------------------------------------------------ (a) the helper
@pytest.mark.parametrize("axes", [None, AXES2], ids=["P3", "P2"])
def test_helper_matrix_equals_the_packages_host_matrix(axes):
    emu = _emulator(3, axes)
    m, (M, P) = emu.ncomps, emu.grid_points.shape
    assert list(emu.hyperparams) == ED.labels(m, P) == emu.gradient_labels
    row = displaced_row(emu)
    V, D = ED.slot_derivatives(emu.grid_points, emu.iPhiPhi, row)
    assert V.dtype == np.float64 and [k for k, _ in D] == emu.gradient_labels
    want = emu.iPhiPhi / np.exp(row[0]) + batch_kernel(emu.grid_points, emu.grid_points, np.exp(row[1:1 + m]),
                                                        np.exp(row[1 + m:]).reshape(m, P))
    # the two order the operations differently ((x_g - x_h) / l here, x_g / l - x_h / l scaled per row there): the exponent, at
    # most 1.3 at these lengthscales, is off by a few eps of itself and exp hands that on: 16 eps
    np.testing.assert_allclose(V, want, rtol=16 * np.finfo(np.float64).eps, atol=0)
    assert ED.slot_derivatives(emu.grid_points, emu.iPhiPhi, row, LD)[0].dtype == LD


@pytest.mark.parametrize("axes", [None, AXES2], ids=["P3", "P2"])
def test_helper_derivatives_agree_with_a_stencil_of_its_own_matrix(axes):
    """Tolerance 1e-8 max|D|: the stencil's truncation at step 1e-3 is about 1e-12 (the RBF is smooth: nothing is left out),
    a missing term or a slot in the wrong place is an error of order 1."""
    emu = _emulator(2, axes)
    row = displaced_row(emu).astype(LD)
    h = LD(1e-3)
    _, D = ED.slot_derivatives(emu.grid_points, emu.iPhiPhi, row, LD)
    assert len(D) == row.size
    for s, (name, d) in enumerate(D):
        def V_of(x):
            r = row.copy()
            r[s] = x
            return ED.slot_derivatives(emu.grid_points, emu.iPhiPhi, r, LD)[0]

        assert d.dtype == LD and np.abs(d).max() > 0
        rel = float(np.abs(stencil(V_of, row[s], h) - d).max() / np.abs(d).max())
        print(f"{name}: max |stencil - D| = {rel:.3g} max|D|")
        assert rel <= 1e-8, (name, rel)


# ------------------------------------------------------------------ (b) the identity
@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_contraction_is_the_gradient_of_the_host_likelihood(shape):
    """Longdouble throughout (u = 5e-20).  The stencil at h = 1e-3 is held to 1e-9 (|g|_max + 1): its truncation h^4 / 30
    |f^(5)| is about 3e-14 |f^(5)|, its rounding u cond |lnL| / h about 1e-10 at cond = 3e5 and |lnL| of a few thousand;
    central differences of the float64 likelihood stop at 1e-6.  Eight slots of the largest shape, every slot of the others:
    lambda_xi, the first and last variance and lengthscales of the first and last component."""
    m, axes = SHAPES[shape]
    emu = _emulator(m, axes)
    M, P = emu.grid_points.shape
    n = m * M
    row = displaced_row(emu).astype(LD)
    lnl, g = ED.gradient(emu.grid_points, emu.iPhiPhi, emu.w_hat, row, LD)
    assert abs(float(lnl - ED.log_likelihood(ED.slot_derivatives(emu.grid_points, emu.iPhiPhi, row, LD)[0], emu.w_hat))) <= 1e-12 * abs(float(lnl))
    slots = range(row.size) if n < 200 else [0, 1, m, 1 + m, 2 + m, m + P, row.size - 2, row.size - 1]
    scale = float(np.abs(g).max()) + 1
    for s in slots:
        def f(x):
            r = row.copy()
            r[s] = x
            return ED.log_likelihood(ED.slot_derivatives(emu.grid_points, emu.iPhiPhi, r, LD)[0], emu.w_hat)

        fd = stencil(f, row[s], LD(1e-3))
        err = abs(float(g[s] - fd))
        print(f"{shape} {emu.gradient_labels[s]}: identity {float(g[s]):.12g}, stencil {float(fd):.12g}, |diff| / (|g|_max + 1) = {err / scale:.3g}")
        assert err <= 1e-9 * scale, (shape, s, float(g[s]), float(fd))
    # the lambda_xi slot as -1/2 alpha^T (iPhiPhi / lambda) alpha + 1/2 (n - tr(G K)): correct but cancelling (K is 1e4 times
    # iPhiPhi), so a cross-check in longdouble only
    V, D = ED.slot_derivatives(emu.grid_points, emu.iPhiPhi, row, LD)
    _, G, alpha = ED.inverse_and_solve(V, emu.w_hat)
    K = V + D[0][1]  # V - iPhiPhi / lambda
    other = (alpha @ (D[0][1] @ alpha) + (n - np.sum(G * K))) / 2
    print(f"{shape}: lambda_xi slot {float(g[0]):.15g}, by n - tr(G K) {float(other):.15g}")
    assert abs(float(g[0] - other)) <= 1e-12 * n


# ------------------------------------------------------------------ (c) refusals
NEW = ("sf_emulator_loglike_grad_workspace_bytes", "sf_emulator_loglike_grad_batch", "sf_debug_emulator_grad_contract")


def test_the_new_entry_points_are_declared_and_bound_with_matching_argument_counts():
    header = open(os.path.join(ROOT, "include", "starfish_amd.h")).read()
    lib = _lib.load()
    for name in NEW:
        found = re.findall(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", header)
        assert len(found) == 1, f"{name} is not declared (once) in include/starfish_amd.h"
        nargs = len([a for a in found[0].split(",") if a.strip() and a.strip() != "void"])
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name


P256 = 1 << 20  # a dummy, 256-byte aligned "device pointer": a refused call never touches it
GOOD = dict(grid=P256, M=27, P=3, m=2, hyper=P256, hyper_stride=9, B=3, iphiphi=P256, w_hat=P256, lnl=P256, grad=P256,
            grad_stride=9, info=P256, work=P256)
BAD = {
    "null grid": dict(grid=None),
    "null hyper": dict(hyper=None),
    "null iphiphi": dict(iphiphi=None),
    "null w_hat": dict(w_hat=None),
    "null lnl": dict(lnl=None),
    "null grad": dict(grad=None),
    "null info": dict(info=None),
    "null workspace": dict(work=None),
    "no grid axis": dict(P=0, hyper_stride=9),
    "nine grid axes": dict(P=9, hyper_stride=21, grad_stride=21),
    "hyper rows shorter than the slots": dict(hyper_stride=8),
    "gradient rows shorter than the slots": dict(grad_stride=8),
    "no row": dict(B=0),
    "negative batch": dict(B=-2),
    "more rows than a grid plane": dict(B=65536),
    "misaligned workspace": dict(work=P256 + 8),
}


def grad_call(lib, work_bytes=None, **kw):
    a = dict(GOOD, **kw)
    if work_bytes is None:
        work_bytes = 1 << 40
    return lib.sf_emulator_loglike_grad_batch(a["grid"], a["M"], a["P"], a["m"], a["hyper"], a["hyper_stride"], a["B"], a["iphiphi"],
                                              a["w_hat"], a["lnl"], a["grad"], a["grad_stride"], a["info"], a["work"], work_bytes,
                                              None)


@pytest.mark.parametrize("case", list(BAD))
def test_loglike_grad_refuses_bad_arguments_before_anything_is_enqueued(case):
    lib = _lib.load()
    assert grad_call(lib, **BAD[case]) == SF_EINVAL, case
    assert lib.sf_last_error().decode().startswith("sf_emulator_loglike_grad_batch:"), (case, lib.sf_last_error())


def test_workspace_query_and_the_short_workspace():
    lib = _lib.load()
    q = lib.sf_emulator_loglike_grad_workspace_bytes
    M, P, m, B = 27, 3, 2, 3
    npad, nbr, slots = 64, 1, 9
    need = q(M, P, m, B)
    base = lib.sf_emulator_loglike_workspace_bytes(M, m, B)
    a256 = lambda x: -(-x // 256) * 256  # noqa: E731
    # behind the likelihood's layout: alpha, the workspace of sf_potri_blocks_batch, one double per (row, block row, slot)
    assert need == a256(a256(base) + 8 * B * npad) + lib.sf_potri_blocks_workspace_bytes(npad, B) + 8 * B * nbr * slots
    assert q(M, P, m, B + 1) > need > q(M, P, m, B - 1) > 0
    assert q(M, 2, m, B) < need  # fewer slots
    for bad in ((0, P, m, B), (M, 0, m, B), (M, 9, m, B), (M, P, 0, B), (M, P, m, 0), (M, P, m, 65536), (M, -1, m, B)):
        assert q(*bad) == 0, bad
    assert grad_call(lib, work_bytes=need - 1) == SF_ENOMEM
    assert b"workspace" in lib.sf_last_error()
    a = GOOD
    rc = lib.sf_debug_emulator_grad_contract(a["grid"], M, P, m, a["hyper"], 9, B, a["iphiphi"], a["grad"], 8, a["info"], a["work"],
                                             need, None)
    assert rc == SF_EINVAL and lib.sf_last_error().decode().startswith("sf_debug_emulator_grad_contract:")


# ------------------------------------------------------------------ (d) train(gradient=True) over a stand-in evaluator
class HostGradient:
    """A host log_likelihood_gradient_batch: the helper's identity in float64; fails (info 7) where `fail(x)` says so."""

    def __init__(self, emu, fail=None):
        self.emu, self.fail, self.rows = emu, fail, []

    def __call__(self, X, return_info=False):
        assert return_info
        X = np.atleast_2d(X)
        lnl, grad, info = np.empty(len(X)), np.empty(X.shape), np.zeros(len(X), dtype=np.int32)
        for b, x in enumerate(X):
            self.rows.append(x.copy())
            if self.fail is not None and self.fail(x):
                lnl[b], grad[b], info[b] = -np.inf, np.nan, 7
            else:
                lnl[b], grad[b] = ED.gradient(self.emu.grid_points, self.emu.iPhiPhi, self.emu.w_hat, x)
        return lnl, grad, info


class Quadratic:
    """lnL = -1/2 |x - target|^2: an optimiser's end point is known."""

    def __init__(self, target):
        self.target, self.rows = target, []

    def __call__(self, X, return_info=False):
        X = np.atleast_2d(X)
        self.rows.append(X[0].copy())
        return -0.5 * np.sum((X - self.target) ** 2, axis=1), -(X - self.target), np.zeros(len(X), dtype=np.int32)


def test_the_wall_of_the_simplex_objective_becomes_a_bound_per_lengthscale():
    emu = _emulator(2)
    keys = emu.gradient_labels
    b = emu._lengthscale_bounds()
    assert isinstance(b, Bounds)
    for i, k in enumerate(keys):
        if k.startswith("log_lengthscale:"):
            assert b.lb[i] == np.log(2 * emu._grid_sep[int(k.split(":")[2])]) and b.ub[i] == np.inf
        else:
            assert b.lb[i] == -np.inf and b.ub[i] == np.inf
    # the optimum of the stand-in lies below the wall in every lengthscale: the search ends ON the bound
    target = emu.get_param_vector() - 1.0
    emu.log_likelihood_gradient_batch = Quadratic(target)
    soln = emu.train(gradient=True)
    assert soln.success and emu._trained is True
    ls = np.array([k.startswith("log_lengthscale:") for k in keys])
    np.testing.assert_array_equal(soln.x[ls], b.lb[ls])
    np.testing.assert_allclose(soln.x[~ls], target[~ls], atol=1e-5)
    np.testing.assert_array_equal(emu.get_param_vector(), soln.x)
    for x in emu.log_likelihood_gradient_batch.rows:
        assert np.all(x >= b.lb)


def test_bounds_of_the_caller_are_intersected_with_the_wall():
    emu = _emulator(2)
    keys = emu.gradient_labels
    wall = emu._lengthscale_bounds()
    i_ls, i_lam = keys.index("log_lengthscale:1:0"), keys.index("log_lambda_xi")
    P0 = emu.get_param_vector()
    pairs = [(None, None)] * len(keys)
    pairs[i_ls] = (wall.lb[i_ls] + 0.2, None)       # tighter than the wall: the caller's holds
    pairs[i_ls + 1] = (wall.lb[i_ls + 1] - 5.0, None)  # looser than the wall: the wall holds
    pairs[i_lam] = (None, P0[i_lam] - 0.5)
    for given in (pairs, Bounds([-np.inf if a is None else a for a, _ in pairs], [np.inf if c is None else c for _, c in pairs])):
        got = emu._lengthscale_bounds(given)
        assert got.lb[i_ls] == wall.lb[i_ls] + 0.2 and got.lb[i_ls + 1] == wall.lb[i_ls + 1]
        assert got.ub[i_lam] == P0[i_lam] - 0.5 and got.lb[i_lam] == -np.inf
    emu.log_likelihood_gradient_batch = Quadratic(P0 - 1.0)
    soln = emu.train(gradient=True, bounds=pairs)
    assert soln.success
    assert soln.x[i_ls] == wall.lb[i_ls] + 0.2 and soln.x[i_ls + 1] == wall.lb[i_ls + 1]
    np.testing.assert_allclose(soln.x[i_lam], P0[i_lam] - 1.0, atol=1e-5)
    with pytest.raises(ValueError):
        emu._lengthscale_bounds([(None, None)] * (len(keys) - 1))
    upper = [(None, None)] * len(keys)
    upper[i_ls] = (None, wall.lb[i_ls] - 0.1)
    with pytest.raises(ValueError, match="twice the grid separation"):
        emu.train(gradient=True, bounds=upper)


def test_gradient_and_batch_simplex_exclude_each_other():
    emu = _emulator(2)
    emu.log_likelihood_gradient_batch = emu.log_likelihood_batch = None  # (neither is reached)
    with pytest.raises(ValueError, match="batch_simplex"):
        emu.train(gradient=True, batch_simplex=True)


def test_gradient_train_over_the_host_likelihood_climbs_and_leaves_the_emulator_as_the_serial_loop_does():
    emu = _emulator(2)
    P0 = emu.get_param_vector()
    ev = emu.log_likelihood_gradient_batch = HostGradient(emu)
    start = ED.gradient(emu.grid_points, emu.iPhiPhi, emu.w_hat, P0)[0]
    soln = emu.train(gradient=True)
    print(f"L-BFGS-B over the host gradient: {soln.message}; nit {soln.nit}, nfev {soln.nfev}; lnL {start!r} -> {-soln.fun!r}")
    assert soln.success and emu._trained is True and -soln.fun > start
    assert soln.nfev == len(ev.rows)
    np.testing.assert_array_equal(emu.get_param_vector(), soln.x)
    # an optimiser that stops early: not a success, the emulator stands at the last point the objective was asked for
    emu = _emulator(2)
    ev = emu.log_likelihood_gradient_batch = HostGradient(emu)
    soln = emu.train(gradient=True, options=dict(maxiter=1))
    assert not soln.success and emu._trained is False
    np.testing.assert_array_equal(emu.get_param_vector(), ev.rows[-1])
    # a point whose v11 is not positive definite: the scalar path's error, the emulator at that point
    emu = _emulator(2)
    ev = emu.log_likelihood_gradient_batch = HostGradient(emu, fail=lambda x: len(ev.rows) >= 3)
    with pytest.raises(np.linalg.LinAlgError, match="7-th leading minor of the array is not positive definite"):
        emu.train(gradient=True)
    assert emu._trained is False and len(ev.rows) == 3
    np.testing.assert_array_equal(emu.get_param_vector(), ev.rows[-1])


def test_the_default_train_never_calls_the_gradient():
    emu = _emulator(2)
    calls = []

    def scalar():
        calls.append(1)
        return float(ED.gradient(emu.grid_points, emu.iPhiPhi, emu.w_hat, emu.get_param_vector())[0])

    def never(*a, **k):
        raise AssertionError("the gradient must not run on the default path")

    emu.log_likelihood = scalar
    emu.log_likelihood_gradient_batch = never
    soln = emu.train(options=dict(maxiter=3))
    assert calls and soln.nit == 3


def test_scalar_gradient_is_the_batch_row_and_raises_as_the_likelihood_does():
    emu = _emulator(2)
    ev = emu.log_likelihood_gradient_batch = HostGradient(emu)
    lnl, g = emu.log_likelihood_gradient()
    want = ED.gradient(emu.grid_points, emu.iPhiPhi, emu.w_hat, emu.get_param_vector())
    assert lnl == want[0] and g.shape == (len(emu.gradient_labels),)
    np.testing.assert_array_equal(g, want[1])
    np.testing.assert_array_equal(ev.rows[0], emu.get_param_vector())
    emu.log_likelihood_gradient_batch = HostGradient(emu, fail=lambda x: True)
    with pytest.raises(np.linalg.LinAlgError, match="7-th leading minor"):
        emu.log_likelihood_gradient()
    # a matrix assigned by hand has no hyper-parameter row (checked before the device is asked for)
    emu = _emulator(2)
    emu.v11 = emu.v11 + 0.5 * np.eye(len(emu.v11))
    with pytest.raises(ValueError, match="assigned by hand"):
        emu.log_likelihood_gradient_batch(emu.get_param_vector())
