"""The multi-order calls -- likelihood, gradient, gradient and Fisher information on the band solver -- compute bit for bit what
they computed before their host layer was regrouped around one lane / chunk pipeline (csrc/sf_multi_pipeline.h) and their plans
around one frame (starfish_amd/_multi.py): tests/golden/multi_bits.json is the output of tools/multi_bits.py on the tree BEFORE
that change (sha256 of every returned array per order, of the order sums, and the plans' call counts, half-widths and re-routed
units), and the tree must reproduce every entry -- an equality, no tolerance.

Cases: the tool's docstring.  Its last group has 400 units in four segments: the first chunk of the pipeline closes behind the
third segment, a second chunk exists and lane 0 is used twice; for its likelihood every order's values are also held against the
order's own single-order call.  Needs an MI355X: run with -m gpu."""
import importlib.util
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT


@pytest.fixture(scope="module")
def multi_bits():
    spec = importlib.util.spec_from_file_location("multi_bits", os.path.join(ROOT, "tools", "multi_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def want():
    with open(os.path.join(GOLDEN, "multi_bits.json")) as f:
        return json.load(f)


GROUPS = ["likelihood", "gradient", "banded-gradient", "banded-fisher", "two-chunk"]


def test_fixture_holds_every_group(want, multi_bits):
    assert list(multi_bits.GROUPS) == GROUPS
    assert sorted({k.split(":")[0] for k in want}) == sorted(GROUPS)
    cases = {k.split("/")[0] for k in want}
    assert len(cases) == 4 + 3 + 9 + 9 + 4  # the cases of the tool's docstring, group by group
    for entry in ("two-chunk:two-chunk-banded-grad/complete", "two-chunk:two-chunk-banded-fisher/complete"):
        assert want[entry] == 1  # all 400 units ran on the band kernels


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS)
def test_multi_order_bits_match_the_tree_before(multi_bits, want, group):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    got = {}
    multi_bits.GROUPS[group](got)
    got = {f"{group}:{k}": v for k, v in got.items()}
    expect = {k: v for k, v in want.items() if k.startswith(group + ":")}
    assert sorted(got) == sorted(expect)
    differ = sorted(k for k in expect if got[k] != expect[k])
    assert not differ, f"entries that differ from the tree before: {differ}"


@pytest.mark.gpu
def test_two_chunk_likelihood_agrees_with_every_orders_own_call(multi_bits):
    """400 units in two chunks against each order's single-order ``loglike``: the bound of tests/test_gpu_echelle_per_order.py."""
    from starfish_amd import _device as D

    _, models, em, P = multi_bits.two_chunk_model()
    devs, mds, rows = multi_bits.pack(models, P, em._layout()[1])
    assert sum(len(r) for r in rows) == 400 and sum(len(r) for r in rows[:2]) < 256 <= sum(len(r) for r in rows[:3])
    for i, (out, dev, md, r) in enumerate(zip(D.loglike_multi(devs, mds, rows), devs, mds, rows)):
        own = dev.loglike(md, r)
        assert (out["info"] == 0).all() and (own["info"] == 0).all(), (i, out["info"], own["info"])
        np.testing.assert_allclose(out["lnl"], own["lnl"], rtol=1e-12, atol=0, err_msg=f"order {i}")
