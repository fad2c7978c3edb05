"""Host side of the covariance gradient on the band solver (no device): the new C-ABI names, what the calls refuse before they
touch the device, the block recurrence of the selected inversion (tests/band_selinv_reference.py) against a dense inverse, the
identity 1/2 sum_band (alpha alpha^T - Sigma + Vs Vs^T) D = 1/2 sum (alpha alpha^T - C^-1) D, and the SpectrumModel refusals."""
import os
import re

import numpy as np
import pytest

from starfish_amd import _lib, synth
from starfish_amd.models import SpectrumModel

import band_selinv_reference as SR
import banded_derivatives as BD
import cov_derivatives as CD
from gpu_helpers import oracle_order

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
NEW_NAMES = {"sf_band_selinv_workspace_bytes": 3, "sf_band_selinv_batch": 14, "sf_loglike_banded_grad_workspace_bytes": 6,
             "sf_loglike_banded_grad_batch": 16}
EINVAL, ENOMEM, FAKE = -1, -2, 4096  # (a pointer that is not NULL; the calls below return before they read it)
LD = np.longdouble
SHAPES = [(16, 0), (40, 60), (64, 63), (100, 5), (257, 16), (257, 37), (333, 80), (300, 128), (500, 144), (180, 119)]


def test_new_entry_points_are_declared_bound_and_exported():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "starfish_amd.h")).read()
    for name, nargs in NEW_NAMES.items():
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        declared = re.search(rf"\b{name}\s*\(([^;]*)\);", header)
        assert declared and declared.group(1).count(",") + 1 == nargs, name


def test_workspace_queries_return_zero_for_what_the_calls_refuse():
    lib = _lib.load()
    assert lib.sf_band_selinv_workspace_bytes(300, 144, 3) > 0
    for n, w, batch in ((0, 16, 3), (300, -1, 3), (300, 16, 0), (300, 145, 3), (300, 160, 3)):
        assert lib.sf_band_selinv_workspace_bytes(n, w, batch) == 0, (n, w, batch)
    # the factor's band with one block of right-hand sides: n (nbr + 1) 16 doubles per matrix, nbr = 9 at W = 120
    per = lib.sf_band_selinv_workspace_bytes(4096, 120, 2) - lib.sf_band_selinv_workspace_bytes(4096, 120, 1)
    assert 4096 * 160 * 8 <= per <= 4096 * 160 * 8 + 512
    md = _lib.ModelDesc()
    for want_cov in (0, 1):
        assert lib.sf_loglike_banded_grad_workspace_bytes(None, _lib.C.byref(md), 3, 100, 2, want_cov) == 0
        assert lib.sf_loglike_banded_grad_workspace_bytes(None, None, 3, 100, 0, want_cov) == 0


def selinv_rc(lib, n=300, w=16, ldb=18, ldo=18, batch=3, band=FAKE, out=FAKE, logdet=FAKE, info=FAKE, work=FAKE, have=1 << 40):
    return lib.sf_band_selinv_batch(band, n, w, ldb, n * ldb, batch, out, ldo, n * ldo, logdet, info, work, have, None)


def test_band_selinv_refuses_before_any_device_call():
    lib = _lib.load()
    for kw, word in ((dict(w=160, ldb=162, ldo=162), "window"), (dict(w=145, ldb=146, ldo=146), "window"), (dict(band=None), "null"),
                     (dict(out=None), "null"), (dict(logdet=None), "null"), (dict(info=None), "null"), (dict(work=None), "null"),
                     (dict(ldb=16), "ldb"), (dict(ldo=16), "ldo"), (dict(n=0), "n=0"), (dict(batch=0), "batch=0")):
        assert selinv_rc(lib, **kw) == EINVAL, kw
        assert word in lib.sf_last_error().decode(), (kw, lib.sf_last_error().decode())
    assert selinv_rc(lib, have=1024) == ENOMEM and "workspace" in lib.sf_last_error().decode()


def grad_rc(lib, halfwidth=100, slots=(2,), nslots=None, want_cov=1, params=FAKE, lnl=FAKE, grad=FAKE, work=FAKE):
    nslots = len(slots) if nslots is None else nslots
    h_slots = (_lib.C.c_int * max(len(slots), 1))(*slots) if slots is not None else None
    md = _lib.ModelDesc()
    return lib.sf_loglike_banded_grad_batch(None, _lib.C.byref(md), 3, params, halfwidth, h_slots, nslots, want_cov, lnl, grad, 8,
                                            None, None, work, 1 << 40, None)


def test_banded_grad_refuses_before_any_device_call():
    """Without a context: what the call refuses before it looks at one, and that it never gets past it."""
    lib = _lib.load()
    for kw, word in ((dict(params=None), "required"), (dict(lnl=None), "required"), (dict(grad=None), "required"),
                     (dict(work=None), "required"), (dict(slots=None, nslots=2), "h_slots"),
                     (dict(slots=(), want_cov=0), "nothing to differentiate"), (dict(slots=None, nslots=0, want_cov=0), "nothing"),
                     (dict(halfwidth=160), "sf_loglike_grad_batch"), (dict(halfwidth=145), "LDS window"), (dict(halfwidth=-1), "half-width")):
        assert grad_rc(lib, **kw) == EINVAL, kw
        assert word in lib.sf_last_error().decode(), (kw, lib.sf_last_error().decode())
    assert grad_rc(lib) == EINVAL  # (no context)
    assert grad_rc(lib, slots=None, nslots=0) == EINVAL


# ------------------------------------------------------------------------------------------ the recurrence
@pytest.mark.parametrize("n,w", SHAPES)
def test_block_recurrence_agrees_with_a_dense_inverse_on_the_band(n, w):
    """longdouble: against the dense longdouble inverse X = Xl^T Xl, Xl = L^-1 by substitution.  Both invert the same matrix
    backward-stably in longdouble, so they differ by at most 2 c n eps_ld cond(A) max|X| (c a small constant: 8); the matrices
    are strictly diagonally dominant, cond(A) <= a few tens.  float64: within the entrywise bound the device's band is held to
    (selinv_bound, from the longdouble factor alone) of the longdouble recurrence."""
    rng = np.random.default_rng(100 * n + w)
    A, band, ldb = SR.band_spd(rng, n, w)
    assert band.shape == (n, ldb) and ldb >= w + 1
    ref = SR.selected_inverse(A.astype(LD), w, LD)
    Xl = SR.inverse_lower(SR.cholesky(A.astype(LD)))
    X = Xl.T @ Xl
    mask = SR.on_band(n, w)
    scale = float(np.abs(X).max())
    err = float(np.abs(ref["band"] - SR.band_of(X, w))[mask].max())
    tol = 16 * n * float(np.finfo(LD).eps) * np.linalg.cond(A) * scale
    print(f"n={n} w={w}: longdouble recurrence vs dense inverse {err / scale:.3g} of the largest entry (tolerance {tol / scale:.3g})")
    assert err <= tol
    assert float(np.abs(ref["L"] @ ref["L"].T - A).max()) <= 16 * n * float(np.finfo(LD).eps) * np.abs(A).max()
    got = SR.selected_inverse(A, w)
    bound = SR.selinv_bound(A, w, ref["L"])
    ratio = (np.abs(got["band"] - ref["band"].astype(np.float64))[mask] / bound[mask]).max()
    err64 = float(np.abs(got["band"] - SR.band_of(np.linalg.inv(A), w))[mask].max())
    print(f"n={n} w={w}: float64 recurrence: largest err / bound {ratio:.3g}; against numpy.linalg.inv {err64 / scale:.3g} of the largest entry")
    assert ratio <= 1.0
    assert (got["band"][~mask] == 0).all()


# ------------------------------------------------------------------------------------------ the identity
def test_band_contraction_equals_the_dense_formula_in_longdouble():
    """One small order whose band (log_ls = log 1.5) is narrower than the matrix.  Both sides are longdouble; they take the
    inverse of two float64 data sets that differ by the roundings of the oracle's C = X^T Sigma_w^-1 X + ... (see
    tests/test_banded_gradient_host.py): relative difference at most cond(C) cond(Sigma_w) gamma_{m+8} + 4 N cond(C) eps_ld of
    1/2 sum |A| Dbar per slot."""
    o = synth.make_order(N=64, m=4, seed=5)
    oo = oracle_order(o)
    p = synth.vector_to_oracle_params(synth.walker_ball(o, B=1, seed=3)[0])
    p["global_cov"] = (p["global_cov"][0], float(np.log(1.5)))
    q = BD.pieces(oo, p)
    N, m = len(q["r"]), q["X"].shape[0]
    w = BD.halfwidth(q["Bd"])
    assert 0 < w < N - 1
    wave = o["wave"]
    D = CD.slot_derivatives(wave, p, dtype=LD)
    Dbar = CD.slot_derivatives(wave, p, absolute=True)
    for (_, d) in D:  # the derivative has the support of the kernel: inside the band
        i, j = np.nonzero(np.asarray(d, dtype=np.float64))
        assert np.abs(i - j).max() <= w
    Xl = SR.inverse_lower(SR.cholesky(q["C"].astype(LD)))
    Cinv = Xl.T @ Xl
    alpha = Cinv @ q["r"].astype(LD)
    A = np.outer(alpha, alpha) - Cinv
    got = SR.banded_cov_gradient(q, D, w)
    assert [label for label, _ in got] == [label for label, _ in D] and len(D) == 5
    tol = np.linalg.cond(q["C"]) * np.linalg.cond(q["S"]) * SR.gamma(m + 8) + 4 * N * np.linalg.cond(q["C"]) * float(np.finfo(LD).eps)
    for (label, g), (_, d), (_, dbar) in zip(got, D, Dbar):
        want = 0.5 * np.sum(A * d)
        size = 0.5 * float(np.sum(np.abs(A) * dbar))
        rel = abs(float(g - want)) / size
        print(f"{label}: band {float(g)!r}, dense {float(want)!r}, relative difference {rel:.3g} (tolerance {tol:.3g})")
        assert rel <= tol


# ------------------------------------------------------------------------------------------ the model's refusals
def test_model_refuses_an_unknown_covariance_solver_and_one_pass_on_the_band_solver(monkeypatch):
    def refuse(self):
        raise AssertionError("the host logic asked for a device")

    monkeypatch.setattr(SpectrumModel, "_device", refuse)
    model = synth.build_model(synth.make_order(N=64, m=4, seed=5))
    P = model.get_param_vector()[None, :]
    for call in (lambda: model.log_likelihood_gradient(solver="sparse"),
                 lambda: model.log_likelihood_gradient_batch(P, solver="sparse"),
                 lambda: model.log_likelihood_full_gradient_batch(P, covariance_solver="sparse"),
                 lambda: model.train_covariance(gradient_solver="sparse"),
                 lambda: model.train(gradient=True, covariance_solver="sparse")):
        with pytest.raises(ValueError, match="solver"):
            call()
    for solver in ("auto", "banded"):
        with pytest.raises(ValueError, match="one_pass"):
            model.log_likelihood_full_gradient_batch(P, one_pass=True, covariance_solver=solver)
    with pytest.raises(TypeError):
        model.train(None, True, True, None, "auto")  # (the new argument is keyword only)
