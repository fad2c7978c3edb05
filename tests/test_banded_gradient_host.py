"""Host side of the mean-flux gradient on the band + Woodbury solver (no device): the new C-ABI names, what the calls refuse
before they touch the device, the shape helpers of the full banded solve against a restatement in Python, the identity
[alpha, V] = Bd^-1 [r, Y^T] M against the dense solve of tests/mean_derivatives.py, and the SpectrumModel refusals."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from starfish_amd import _lib, synth
from starfish_amd.models import SpectrumModel

import banded_derivatives as BD
import mean_derivatives as MD
from gpu_helpers import oracle_order

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CSRC = os.path.join(ROOT, "starfish_amd", "csrc")
NEW_NAMES = {"sf_band_solve_workspace_bytes": 4, "sf_band_solve_batch": 19, "sf_loglike_banded_mean_grad_workspace_bytes": 5,
             "sf_loglike_banded_mean_grad_batch": 15}
EINVAL, FAKE = -1, 4096  # (a pointer that is not NULL; the calls below return before they read it)


def test_new_entry_points_are_declared_bound_and_exported():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "starfish_amd.h")).read()
    for name, nargs in NEW_NAMES.items():
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        declared = re.search(rf"\b{name}\s*\(([^;]*)\);", header)
        assert declared and declared.group(1).count(",") + 1 == nargs, name


def test_workspace_queries_return_zero_for_bad_arguments():
    lib = _lib.load()
    assert lib.sf_band_solve_workspace_bytes(300, 128, 3, 17) > 0
    for n, w, batch, nrhs in ((0, 16, 3, 1), (300, -1, 3, 1), (300, 16, 0, 1), (300, 16, 3, 0), (300, 16, 3, 49), (300, 160, 3, 1),
                              (300, 144, 3, 17), (300, 128, 3, 33)):
        assert lib.sf_band_solve_workspace_bytes(n, w, batch, nrhs) == 0, (n, w, batch, nrhs)
    # about n (W + 16 + 16 nrb) doubles per matrix: the factor's band, one block of slack, the right-hand sides
    per = lib.sf_band_solve_workspace_bytes(4096, 120, 2, 5) - lib.sf_band_solve_workspace_bytes(4096, 120, 1, 5)
    assert 4096 * (120 + 16 + 5) * 8 <= per <= 4096 * (120 + 32 + 16) * 8 + 512
    md = _lib.ModelDesc()
    assert lib.sf_loglike_banded_mean_grad_workspace_bytes(None, _lib.C.byref(md), 3, 100, 2) == 0
    assert lib.sf_loglike_banded_mean_grad_workspace_bytes(None, None, 3, 100, 2) == 0


def solve_rc(lib, n=300, w=16, ldb=18, batch=3, nrhs=2, band=FAKE, rhs=FAKE, x=FAKE, logdet=FAKE, info=FAKE, work=FAKE, have=1 << 40):
    return lib.sf_band_solve_batch(band, n, w, ldb, n * ldb, batch, rhs, nrhs, n, nrhs * n, x, n, nrhs * n, logdet, None, info, work,
                                   have, None)


def test_band_solve_refuses_before_any_device_call():
    lib = _lib.load()
    for kw, word in ((dict(w=160, ldb=162, nrhs=1), "window"), (dict(w=144, ldb=146, nrhs=17), "window"), (dict(nrhs=49), "nrhs"),
                     (dict(nrhs=0), "nrhs"), (dict(x=None), "null"), (dict(band=None), "null"), (dict(work=None), "null"),
                     (dict(info=None), "null"), (dict(ldb=16), "ldb")):
        assert solve_rc(lib, **kw) == EINVAL, kw
        assert word in lib.sf_last_error().decode(), (kw, lib.sf_last_error().decode())
    assert solve_rc(lib, have=1024) == -2 and "workspace" in lib.sf_last_error().decode()  # SF_ENOMEM


# ------------------------------------------------------------------------------------------ shape helpers
BB, BS = 16, 16 * 17


def window_lds_bytes(nbr, nrb):
    NR = nrb * BB
    return 8 * ((nbr * (nbr + 1) // 2) * BS + nrb * nbr * BS + 2 * BS + NR * (NR + 1) + 2 * BB + BB + 8 + 64 + 8)


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    exe = str(tmp_path_factory.mktemp("band_solve") / "band_solve_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "band_solve_driver.cpp"), "-o", exe],
                   check=True)
    lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.strip().split("\n")
    assert lines[-2].startswith("max")
    return ([[int(v) for v in ln.split()] for ln in lines[:-2]], [int(v) for v in lines[-2].split()[1:]],
            [int(v) for v in lines[-1].split()])


def test_shape_helpers_agree_with_their_restatement(shapes):
    rows, maxhw, (split, max_blocks, lds_max) = shapes
    assert (split, max_blocks, lds_max) == (4, 3, 160 * 1024)
    # the window's own limits are what they were: 144 up to 16 right-hand sides, 128 up to 32, 112 up to 48, none beyond
    assert maxhw == [144] * 16 + [128] * 16 + [112] * 16 + [-1]
    seen = set()
    for w, nrhs, nbr, nrb, wbytes, col_blocks, block32, doubles1000, T, part, ldoubles, lbytes, nwaves, per_wave in rows:
        assert nbr == max(3, (w + 31) // 16) and nrb == (nrhs + 15) // 16 and w <= maxhw[nrhs - 1]
        assert wbytes == window_lds_bytes(nbr, nrb) <= lds_max
        seen.add((nbr, nrb))
        # one record per block column: F_k, nbr - 1 blocks below the diagonal, nrb blocks of right-hand sides, 256 doubles each
        assert col_blocks == nbr + nrb and block32 == (3 * col_blocks + 2) * 256
        assert doubles1000 == 63 * col_blocks * 256
        # the ring of solved blocks, then four partial sums per block of right-hand sides; 17-double rows
        assert (T, part, ldoubles, lbytes) == (0, nrb * nbr * BS, nrb * (nbr + split) * BS, 8 * nrb * (nbr + split) * BS)
        assert lbytes <= lds_max and nwaves == split * nrb and nwaves * 64 <= 1024
        assert per_wave == -(-(nbr - 1) // split) <= max_blocks
    assert seen == {(nbr, 1) for nbr in range(3, 11)} | {(nbr, 2) for nbr in range(3, 10)} | {(nbr, 3) for nbr in range(3, 9)}


# ------------------------------------------------------------------------------------------ the identity
@pytest.fixture(scope="module")
def small():
    o = synth.make_order(N=64, m=4, seed=5)
    oo = oracle_order(o)
    p = synth.vector_to_oracle_params(synth.walker_ball(o, B=1, seed=3)[0])
    p["global_cov"] = (p["global_cov"][0], float(np.log(1.5)))  # a band narrower than the matrix (the ball's is ~118 pixels wide)
    return oo, p, BD.pieces(oo, p)


def test_band_plus_low_rank_is_the_oracles_matrix(small):
    _, _, q = small
    assert 0 < BD.halfwidth(q["Bd"]) < 63
    np.testing.assert_allclose(q["Bd"] + q["Y"].T @ q["Y"], q["C"], rtol=1e-12, atol=1e-12 * np.abs(q["C"]).max())
    np.testing.assert_allclose(q["Lw"] @ q["Y"], q["X"], rtol=1e-12, atol=1e-12 * np.abs(q["X"]).max())


def test_banded_alpha_and_V_solve_the_dense_system(small):
    _, _, q = small
    N = len(q["r"])
    alpha, V = BD.alpha_V(q)
    fac = BD.solve_factor(N)
    cnorm = np.abs(q["C"]).sum(axis=1).max()
    for x, b in [(alpha, q["r"])] + [(V[:, k], q["X"][k]) for k in range(V.shape[1])]:
        res = np.abs(q["C"] @ x - b).max()
        bound = fac * (cnorm * np.abs(x).max() + np.abs(b).max())
        print(f"residual {res:.3g}, bound {bound:.3g}")
        assert res <= bound


def test_banded_alpha_and_V_are_those_of_the_dense_helper_in_longdouble(small):
    oo, p, q = small
    ref = {}
    MD.gradient(oo, p, ("log_scale",), dtype=np.longdouble, pieces=ref)
    alpha, V = BD.alpha_V(q, dtype=np.longdouble)
    # Both are longdouble solves, but not of the same data: the dense helper takes the oracle's C, a float64 matrix whose
    # entries carry the roundings of its formation (the m-term product X^T Sigma_w^-1 X behind a solve with Sigma_w, then
    # sigma^2, the kernels and the jitter: at most m + 8 roundings, times cond(Sigma_w) for the solve), the banded one Bd,
    # X and Sigma_w.  A relative perturbation d of the matrix moves the solution by cond(C) d to first order; on top, the
    # two longdouble solves' own errors, N cond(C) eps each way.
    eps, m, N = float(np.finfo(np.longdouble).eps), q["X"].shape[0], len(q["r"])
    cond, cond_w = np.linalg.cond(q["C"]), np.linalg.cond(q["S"])
    tol = cond * cond_w * BD.gamma(m + 8) + 2 * N * cond * eps
    for got, want in ((alpha, ref["alpha"]), (V, ref["V"])):
        err = float(np.abs(got - want).max() / np.abs(want).max())
        print(f"relative difference {err:.3g}, tolerance {tol:.3g} (cond(C) {cond:.3g}, cond(Sigma_w) {cond_w:.3g})")
        assert err <= tol


# ------------------------------------------------------------------------------------------ the model's refusals
def test_model_refuses_an_unknown_solver_and_one_pass_on_the_band_solver(monkeypatch):
    def refuse(self):
        raise AssertionError("the host logic asked for a device")

    monkeypatch.setattr(SpectrumModel, "_device", refuse)
    model = synth.build_model(synth.make_order(N=64, m=4, seed=5))
    P = model.get_param_vector()[None, :]
    for call in (lambda: model.log_likelihood_mean_gradient(solver="sparse"),
                 lambda: model.log_likelihood_mean_gradient_batch(P, solver="sparse"),
                 lambda: model.log_likelihood_full_gradient_batch(P, solver="sparse"),
                 lambda: model.train(gradient=True, gradient_solver="sparse")):
        with pytest.raises(ValueError, match="solver"):
            call()
    for solver in ("auto", "banded"):
        with pytest.raises(ValueError, match="one_pass"):
            model.log_likelihood_full_gradient_batch(P, one_pass=True, solver=solver)
