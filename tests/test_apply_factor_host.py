"""sf_potrs_batch / sf_apply_batch without a device: every bad argument is refused with SF_EINVAL and a message before
any HIP call (sf_apply_batch: before the context is looked at, as its siblings do), and the size queries that need no
context.  (A context needs a device: what the size query of
sf_apply_batch returns for a real order is checked in tests/test_gpu_apply_factor.py.)"""
import ctypes as C

import pytest

from starfish_amd import _lib

SF_EINVAL = -1
FAKE = 0x10000  # a non-null "device pointer": a refused call never touches it

GOOD = dict(L=FAKE, n=128, lda=128, stride=128 * 128, batch=2, op=3, rhs=FAKE + (1 << 24), nrhs=3, ldr=128,
            rhs_stride=3 * 128, out=FAKE + (1 << 25), ldo=128, out_stride=3 * 128)

BAD = {
    "n not a multiple of 64": dict(n=96, lda=128),
    "n zero": dict(n=0),
    "lda below n": dict(lda=127),
    "ldr below n": dict(ldr=127),
    "ldo below n": dict(ldo=64),
    "no right-hand side": dict(nrhs=0),
    "negative nrhs": dict(nrhs=-1),
    "no matrix": dict(batch=0),
    "op below the range": dict(op=-1),
    "op above the range": dict(op=4),
    "null L": dict(L=0),
    "null rhs": dict(rhs=0),
    "null out": dict(out=0),
    "in place on a shared block": dict(out=GOOD["rhs"], rhs_stride=0),
    "in place with another row stride": dict(out=GOOD["rhs"], ldo=130),
    "in place with another matrix stride": dict(out=GOOD["rhs"], out_stride=4 * 128),
}


def potrs(lib, **kw):
    a = dict(GOOD, **kw)
    return lib.sf_potrs_batch(a["L"], a["n"], a["lda"], a["stride"], a["batch"], a["op"], a["rhs"], a["nrhs"], a["ldr"],
                              a["rhs_stride"], a["out"], a["ldo"], a["out_stride"], None)


@pytest.mark.parametrize("case", list(BAD))
def test_potrs_refuses_bad_arguments_before_any_device_call(case):
    lib = _lib.load()  # loading needs no GPU; a call that reached the HIP runtime here would not return SF_EINVAL
    rc = potrs(lib, **BAD[case])
    assert rc == SF_EINVAL, (case, rc)
    msg = lib.sf_last_error().decode()
    assert msg.startswith("sf_potrs_batch:"), (case, msg)


def test_apply_ops_are_the_headers():
    import os
    import re

    from starfish_amd import _device as D

    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "starfish_amd.h")).read()
    got = {name: int(v) for name, v in re.findall(r"#define SF_APPLY_([A-Z]+) (\d)", header)}
    assert got == {"L": 0, "LINV": 1, "LINVT": 2, "CINV": 3}
    assert {k.upper(): v for k, v in D.APPLY_OPS.items()} == got


APPLY_GOOD = dict(ctx=None, B=4, params=FAKE, op=3, rhs=FAKE + (1 << 20), nrhs=3, ldr=4096, rhs_stride=3 * 4096,
                  out=FAKE + (1 << 24), flux=None, info=None, work=FAKE + (1 << 28), work_bytes=1 << 20)

# refused on the counts, the pointers, op and the right-hand-side conventions: before the context is looked at
APPLY_BAD = {
    "no walker": dict(B=0),
    "negative batch": dict(B=-3),
    "more walkers than a grid plane": dict(B=65536),
    "no right-hand side": dict(nrhs=0),
    "more right-hand sides than a grid row": dict(nrhs=65536),
    "null params": dict(params=None),
    "null out": dict(out=None),
    "op below the range": dict(op=-1),
    "op above the range": dict(op=4),
    "negative rhs stride": dict(rhs_stride=-1),
    "the residual as two right-hand sides": dict(rhs=None, nrhs=2),
}


@pytest.mark.parametrize("case", list(APPLY_BAD))
def test_apply_refuses_bad_arguments_before_it_looks_at_the_context(case):
    lib = _lib.load()  # loading needs no GPU; a call that reached the HIP runtime here would not return SF_EINVAL
    a = dict(APPLY_GOOD, **APPLY_BAD[case])
    rc = lib.sf_apply_batch(a["ctx"], C.byref(_lib.ModelDesc()), a["B"], a["params"], a["op"], a["rhs"], a["nrhs"], a["ldr"],
                            a["rhs_stride"], a["out"], a["flux"], a["info"], a["work"], a["work_bytes"], None)
    assert rc == SF_EINVAL, (case, rc)
    msg = lib.sf_last_error().decode()
    assert msg.startswith("sf_apply_batch:"), (case, msg)


def test_apply_entry_points_refuse_a_missing_context():
    lib = _lib.load()
    md = _lib.ModelDesc()
    assert lib.sf_apply_workspace_bytes(None, C.byref(md), 4, 1) == 0
    rc = lib.sf_apply_batch(None, C.byref(md), 4, FAKE, 3, None, 1, 0, 0, FAKE, None, None, FAKE, 1 << 20, None)
    assert rc == SF_EINVAL and lib.sf_last_error()


def test_the_factorisation_workspace_is_what_it_was():
    """sf_potrs_batch needs no workspace and sf_apply_batch puts its staging area BEHIND the likelihood's layout: the
    pinned sizes of tests/test_host_logic.py hold (restated here for the sizes a 128-walker run meets)."""
    from test_host_logic import POTRF_WORKSPACE_BYTES

    lib = _lib.load()
    for n in (3008, 4096):
        assert [lib.sf_potrf_workspace_bytes(n, b) for b in (1, 16, 64, 128)] == POTRF_WORKSPACE_BYTES[n]
