"""The wide Cholesky sequence (panel pairs, k_chol_panel_w) computes bit for bit what it computed before its epilogue was
rescheduled: tests/golden/potrf_wide_bits.json is the output of tools/potrf_bits.py on the build BEFORE that change (sha256
of the lower triangle of L and of info per matrix; of lnl, logdet, sqmah, info and the residual per walker), and the tree
must reproduce every digest -- an equality, no tolerance: no accumulator's order of operations may change.

Cases (wide sequence pinned, three matrices each): sf_potrf_batch at n = 640 (pair 0 with K = 0, pair 1 with K = 256),
n = 1024 (the stand-alone call takes multiples of 64 only: the order 1000 below, padded) and n = 704 (64 mod 128: the shifted
frame); sf_loglike_batch with one global and one local kernel at N = 640, 1000 and 704 (generated and materialised start tiles,
the right-hand side z of the factor steps).  Needs an MI355X: run with -m gpu."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN, ROOT

CASES = ["potrf-n640", "potrf-n1024", "potrf-n704", "loglike-N640", "loglike-N1000", "loglike-N704"]


@pytest.fixture(scope="module")
def potrf_bits():
    spec = importlib.util.spec_from_file_location("potrf_bits", os.path.join(ROOT, "tools", "potrf_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def want():
    with open(os.path.join(GOLDEN, "potrf_wide_bits.json")) as f:
        return json.load(f)


def test_fixture_holds_every_case(want, potrf_bits):
    assert sorted({k.split("/")[0] for k in want}) == sorted(CASES)
    assert [f"potrf-n{n}" for n in potrf_bits.POTRF_SIZES] + [f"loglike-N{n}" for n in potrf_bits.LOGLIKE_SIZES] == CASES
    for case in CASES:
        per_matrix = 2 if case.startswith("potrf") else 5
        assert sum(k.startswith(case + "/") for k in want) == potrf_bits.BATCH * per_matrix


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_wide_sequence_bits_match_the_build_before(potrf_bits, want, case):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from starfish_amd import _lib

    lib = _lib.require_gpu()
    got = {}
    assert lib.sf_debug_cholesky_sequence(potrf_bits.WIDE) == 0
    try:
        kind, size = case.split("-")
        if kind == "potrf":
            potrf_bits.potrf_case(got, lib, int(size[1:]))
        else:
            potrf_bits.loglike_case(got, int(size[1:]))
    finally:
        lib.sf_debug_cholesky_sequence(-1)
    expect = {k: v for k, v in want.items() if k.startswith(case + "/")}
    assert sorted(got) == sorted(expect)
    differ = sorted(k for k in expect if got[k] != expect[k])
    assert not differ, f"digests that differ from the build before: {differ}"
