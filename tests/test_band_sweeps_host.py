"""Host side of the band sweep's stage tests (no device): tests/band_sweep_reference.py against numpy and against itself, and
what sf_debug_band_forms_batch refuses before it touches the device."""
import os
import re

import numpy as np
import pytest

from starfish_amd import _lib

import band_sweep_reference as SW

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
NEW_NAMES = {"sf_debug_band_forms_workspace_bytes": 5, "sf_debug_band_forms_batch": 17}
EINVAL, ENOMEM, FAKE = -1, -2, 4096  # (a pointer that is not NULL; the calls below return before they read it)


def test_new_entry_points_are_declared_bound_and_exported():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "starfish_amd.h")).read()
    for name, nargs in NEW_NAMES.items():
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        declared = re.search(rf"\b{name}\s*\(([^;]*)\);", header)
        assert declared and declared.group(1).count(",") + 1 == nargs, name


def forms_rc(lib, n=288, w=17, ldb=18, batch=3, nrhs=9, form=1, band=FAKE, rhs=FAKE, logdet=FAKE, gram=FAKE, info=FAKE, work=FAKE,
             have=1 << 40):
    return lib.sf_debug_band_forms_batch(band, n, w, ldb, n * ldb, batch, rhs, nrhs, n, nrhs * n, logdet, gram, info, form, work, have,
                                         None)


def test_debug_band_forms_refuses_before_any_device_call():
    lib = _lib.load()
    for kw, word in ((dict(form=2), "form"), (dict(form=-2), "form"), (dict(n=300), "whole 16-row blocks"),
                     (dict(n=16 * (3 * 3 - 2)), "at least 8"), (dict(n=16 * (3 * 10 - 2), w=144, ldb=146, nrhs=3), "at least 29"),
                     (dict(nrhs=49), "nrhs"), (dict(nrhs=0), "nrhs"), (dict(w=144, ldb=146, nrhs=17, n=960), "window"),
                     (dict(band=None), "null"), (dict(rhs=None), "null"), (dict(logdet=None), "null"), (dict(gram=None), "null"),
                     (dict(info=None), "null"), (dict(work=None), "null"), (dict(work=None, form=-1), "null"), (dict(ldb=17), "ldb"),
                     (dict(nrhs=49, form=0), "nrhs"), (dict(band=None, form=0), "null"), (dict(nrhs=49, form=-1), "nrhs")):
        assert forms_rc(lib, **kw) == EINVAL, kw
        assert word in lib.sf_last_error().decode(), (kw, lib.sf_last_error().decode())
    assert forms_rc(lib, have=1024) == ENOMEM and "workspace" in lib.sf_last_error().decode()
    assert forms_rc(lib, have=1024, form=-1) == ENOMEM


def test_debug_band_forms_workspace_is_the_twisted_layout():
    lib = _lib.load()
    size = lib.sf_debug_band_forms_workspace_bytes
    for n, w, batch, nrhs in ((288, 17, 3, 9), (960, 144, 3, 16), (784, 100, 5, 48)):
        nm, NR, ng = (SW.nbr_of(w) - 1) * 16, -(-nrhs // 16) * 16, nrhs * nrhs
        want = 8 * (batch * (3 * nm * nm + 3 * NR * nm + 3 * ng + 3) + 64)  # (sfb_twist_carve: the dumps twice, the merged once)
        assert size(n, w, batch, nrhs, 1) == size(n, w, batch, nrhs, -1) == want
        assert size(n, w, batch, nrhs, 0) == 0
    assert size(300, 17, 3, 9, -1) > 0  # (the likelihood's choice is then the single sweep; the size does not depend on n)
    for n, w, batch, nrhs, form in ((300, 17, 3, 9, 1), (16 * 7, 17, 3, 9, 1), (288, 17, 3, 49, 1), (288, 17, 0, 9, 1),
                                    (288, 17, 3, 9, 2), (288, -1, 3, 9, -1), (960, 144, 3, 17, -1)):
        assert size(n, w, batch, nrhs, form) == 0, (n, w, batch, nrhs, form)


# ------------------------------------------------------------------------------------------ the helper against numpy
@pytest.mark.parametrize("family,n,w,nrhs", [("dominant", 128, 17, 5), ("matern", 384, 33, 17)])
def test_longdouble_reference_reproduces_numpy(family, n, w, nrhs):
    c = SW.case(family, n, w, nrhs)
    A, rhs = c["A"][0], c["rhs"][0]
    ref = SW.checked(c, 0)["ref"]
    sign, logdet = np.linalg.slogdet(A)
    want = rhs @ np.linalg.solve(A, rhs.T)
    # numpy's own error: its LU / solve are backward stable, so cond(A) times a few n eps bounds it
    cond, eps = np.linalg.cond(A), np.finfo(np.float64).eps
    assert sign > 0 and abs(float(ref["logdet"]) - logdet) <= n * eps * max(1.0, abs(logdet))
    err = np.abs(ref["gram"].astype(np.float64) - want).max() / np.abs(want).max()
    print(f"{family} {n}/{w}/{nrhs}: gram differs from numpy by {err:.3g} relative, cond {cond:.3g}")
    assert err <= 4 * n * eps * cond
    L = ref["L"].astype(np.float64)
    np.testing.assert_allclose(L @ L.T, A, rtol=0, atol=4 * eps * np.abs(A).max())
    np.testing.assert_allclose(A @ ref["X"].astype(np.float64), rhs.T, rtol=0, atol=4 * n * eps * cond * np.abs(rhs).max())


def test_twist_shape_is_the_headers():
    # sfb_twist_shape / sfb_twist_fits (tests/test_hostmath.py holds the header's own values): the table's splits
    assert SW.twist_shape(288, 17) == (32, 8, 8, True)
    assert SW.twist_shape(304, 16) == (32, 8, 9, True)
    assert SW.twist_shape(128, 17) == (32, 3, 3, True) and not SW.twist_shape(112, 17)[3]
    assert SW.twist_shape(992, 144) == (144, 26, 27, True)
    assert SW.twist_shape(464, 144) == (144, 10, 10, True) and not SW.twist_shape(448, 144)[3]
    assert [SW.nbr_of(w) for w in (0, 17, 33, 49, 100, 128, 130, 144)] == [3, 3, 4, 5, 8, 9, 10, 10]


@pytest.mark.parametrize("family,n,w,nrhs", SW.CASES)
def test_float64_eliminations_stay_within_their_bounds(family, n, w, nrhs):
    """Both elimination orders in float64 against the longdouble reference, over the first-order floor alone (the bound
    itself is never below it): the inputs are fair, and the twisted restatement in longdouble is the reference's result."""
    c = SW.case(family, n, w, nrhs)
    for b in range(SW.BATCH):
        k = SW.checked(c, b)
        if k["twisted"] is not None:
            tw, ref = k["twisted"], k["ref"]
            eps = float(np.finfo(SW.LD).eps)
            assert abs(tw["logdet"] - ref["logdet"]) <= k["bounds"][1]["floor_logdet"] * eps * 2.0 ** 53
            assert (np.abs(tw["gram"] - ref["gram"]) <= k["bounds"][1]["floor_gram"] * eps * 2.0 ** 53).all()
            N = tw["N"].astype(np.float64)  # (the product in float64: A = N N^T to float64 rounding)
            assert np.abs(N @ N.T - c["A"][b]).max() <= n * np.finfo(np.float64).eps * np.abs(c["A"][b]).max()
        for form in c["forms"]:
            bd = k["bounds"][form]
            rl, rg = bd["cpu_logdet"] / bd["floor_logdet"], float((bd["cpu_gram"] / bd["floor_gram"]).max())
            print(f"{family} {n}/{w}/{nrhs} matrix {b} form {form}: float64 logdet err / floor {rl:.3g}, gram {rg:.3g}")
            assert rl <= 1 and rg <= 1
            assert bd["logdet"] >= bd["floor_logdet"] and (bd["gram"] >= bd["floor_gram"]).all()
