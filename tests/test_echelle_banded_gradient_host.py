"""Host logic of EchelleModel's gradient on the band solver (no device): the new C-ABI names, what the two entry points
refuse before they look at a context, the ``solver=`` keyword of the model, the per-unit dispatch rule as a pure function, and
the half-width bounds and kink distances of the cases of tests/echelle_banded_cases.py."""
import os
import re

import numpy as np
import pytest

from per_order_cases import PER, per_order_models
from starfish_amd import _device as D
from starfish_amd import _lib
from starfish_amd.models import EchelleModel, SpectrumModel

import echelle_banded_cases as EB

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
NEW_NAMES = {"sf_banded_multi_grad_workspace_bytes_md": 6, "sf_loglike_banded_multi_grad_batch_md": 13}
EINVAL, FAKE = -1, 4096  # (a pointer that is not NULL; the calls below return before they read it)


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    def refuse(self):
        raise AssertionError("the host logic asked for a device")

    monkeypatch.setattr(SpectrumModel, "_device", refuse)


def test_new_entry_points_are_declared_bound_and_exported():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "starfish_amd.h")).read()
    for name, nargs in NEW_NAMES.items():
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        declared = re.search(rf"\b{name}\s*\(([^;]*)\);", header)
        assert declared and declared.group(1).count(",") + 1 == nargs, name
    for name in ("BandedMultiGradPlan", "loglike_banded_multi_grad", "banded_units", "rerouted_units", "merge_units"):
        assert hasattr(D, name), name


def _raw(lib, halfwidths):
    """Both entry points on two segments without a context: (size, return code, message of the call)."""
    segs = (_lib.Segment * 2)()
    for k in range(2):
        segs[k] = _lib.Segment(None, FAKE, 3, 0)
    mds = [_lib.ModelDesc(), _lib.ModelDesc()]
    models = D.MultiPlan._desc_array(mds)
    cols = (_lib.C.c_int32 * 1)(2)
    reqs = (_lib.GradRequest * 2)()
    for k in range(2):
        reqs[k] = _lib.GradRequest(cols, 1, 1)
    h = (_lib.C.c_int * 2)(*halfwidths) if halfwidths is not None else None
    size = lib.sf_banded_multi_grad_workspace_bytes_md(segs, 2, models, reqs, h, 8)
    rc = lib.sf_loglike_banded_multi_grad_batch_md(segs, 2, models, reqs, h, FAKE, None, FAKE, FAKE, 8, FAKE, 1 << 40, None)
    return size, rc, lib.sf_last_error().decode()


def test_half_widths_are_refused_before_a_context_is_looked_at():
    lib = _lib.load()
    for halfwidths, word in ((None, "h_halfwidth"), ((100, -1), "segment 1: half-width -1"), ((160, 100), "segment 0: half-width 160"),
                             ((100, 145), "segment 1: half-width 145")):
        size, rc, msg = _raw(lib, halfwidths)
        assert size == 0 and rc == EINVAL, (halfwidths, size, rc)
        assert "sf_loglike_banded_multi_grad_batch_md" in msg and word in msg, (halfwidths, msg)
        if halfwidths is not None:  # the message names the dense call, as the single-order call names its counterpart
            assert "use sf_loglike_multi_grad_batch_md" in msg and "LDS window" in msg, msg
    # half-widths no window refuses: the call gets as far as the segments, which have no context
    size, rc, msg = _raw(lib, (144, 0))
    assert size == 0 and rc == EINVAL and "segment 0 has no order context" in msg, msg
    assert lib.sf_banded_multi_grad_workspace_bytes_md(None, 2, None, None, None, 8) == 0


def model_with_solver(solver):
    _, models = per_order_models((0, 1, 3), sizes=[64, 130, 180], m=2, seed0=100)
    for m in models:
        m.solver = solver
    return models, EchelleModel.from_orders(models, per_order=PER)


def same_layout(got, want):
    (labels, cols, requests, sources), (labels_w, cols_w, requests_w, sources_w) = got, want
    return (tuple(labels) == tuple(labels_w) and [list(c) for c in cols] == [list(c) for c in cols_w]
            and requests == requests_w and sources == sources_w)


def test_the_solver_keyword_selects_the_gradient_solver_whatever_the_orders_own_is():
    _, dense = model_with_solver("dense")
    want = dense._gradient_layout()
    models, em = model_with_solver("auto")
    for solver in ("dense", "banded", "auto"):
        assert same_layout(em._gradient_layout(solver=solver), want)
        assert same_layout(dense._gradient_layout(solver=solver), want)
    for call in (lambda: em._gradient_layout(), lambda: em._gradient_layout(solver=None),
                 lambda: em.log_likelihood_gradient_batch(np.zeros((1, 32))), lambda: em.log_likelihood_gradient_batch(np.zeros((1, 32)), solver=None),
                 lambda: em.log_likelihood_gradient(), lambda: em.train(), lambda: em.train(gradient_solver=None)):
        with pytest.raises(ValueError, match=r"order 0: the gradient runs on the dense solver only, not solver='auto'"):
            call()
    # the other refusals still come before any device work, under every solver
    models[2].emulator_cov = "paper"
    with pytest.raises(ValueError, match=r'order 2: .*emulator_cov="paper"'):
        em.log_likelihood_gradient_batch(np.zeros((1, 32)), solver="banded")
    with pytest.raises(ValueError, match=r'order 2: .*emulator_cov="paper"'):
        em.train(gradient_solver="auto")


def test_an_unknown_solver_raises_the_message_of_check_solver():
    _, em = model_with_solver("dense")
    message = re.escape("solver must be None, 'dense', 'banded' or 'auto'")
    for call in (lambda: em._gradient_layout(solver="sparse"), lambda: em.log_likelihood_gradient_batch(np.zeros((1, 32)), solver="sparse"),
                 lambda: em.log_likelihood_gradient(solver="window"), lambda: em.train(gradient_solver="sparse")):
        with pytest.raises(ValueError, match=message):
            call()
    with pytest.raises(TypeError):
        em.train(None, "auto")  # (keyword only)


def test_the_dispatch_rule_per_unit():
    """Made-up bounds and codes for three orders of four walkers: windows 144, 144 and 112."""
    bounds = [np.array([100, 144, 145, 480]), np.array([0, 30, 30, 144]), np.array([112, 113, 90, 2**31 - 1])]
    fits = D.banded_units(bounds, [144, 144, 112])
    assert [list(f) for f in fits] == [[True, True, False, False], [True] * 4, [True, False, True, False]]
    # what the band kernels leave: refused units never ran (-4); one flagged -4 by the fill's probe, one -5, one -2, one -1
    infos = [np.array([0, -4, -4, -4]), np.array([-5, 0, -2, 0]), np.array([-1, -4, 0, -4])]
    auto = D.rerouted_units(fits, infos, "auto")
    assert [list(r) for r in auto] == [[1, 2, 3], [0], [1, 3]]
    banded = D.rerouted_units(fits, infos, "banded")
    assert [list(r) for r in banded] == [[], [0], []]  # the internal status alone is recomputed; the rest stays refused
    with pytest.raises(ValueError, match="solver must be"):
        D.rerouted_units(fits, infos, "dense")
    # merging back by (order, walker): only the re-routed rows change, each from its own dense row
    outs = [dict(lnl=np.full(4, float(i)), grad=np.full((4, 2), float(i)), log_scale=np.zeros(4), info=infos[i].copy()) for i in range(3)]
    keep = [{k: v.copy() for k, v in o.items()} for o in outs]
    dense = [dict(lnl=100.0 + 10 * i + np.arange(len(r)), grad=np.full((len(r), 2), 7.0 + i), log_scale=np.ones(len(r)),
                  info=np.zeros(len(r), dtype=np.int64)) for i, r in enumerate(auto)]
    D.merge_units(outs, auto, dense)
    assert list(outs[0]["lnl"]) == [0.0, 100.0, 101.0, 102.0] and list(outs[0]["info"]) == [0, 0, 0, 0]
    assert list(outs[1]["lnl"]) == [110.0, 1.0, 1.0, 1.0] and list(outs[1]["info"]) == [0, 0, -2, 0]
    assert list(outs[2]["lnl"]) == [2.0, 120.0, 2.0, 121.0] and list(outs[2]["info"]) == [-1, 0, 0, 0]
    assert (outs[2]["grad"][[1, 3]] == 9.0).all() and (outs[2]["grad"][[0, 2]] == 2.0).all()
    # orders without a re-routed unit take nothing from the dense list
    outs2 = [{k: v.copy() for k, v in o.items()} for o in keep]
    D.merge_units(outs2, banded, [dict(lnl=np.array([55.0]), grad=np.full((1, 2), 5.0), log_scale=np.ones(1), info=np.zeros(1, dtype=np.int64))])
    assert list(outs2[1]["lnl"]) == [55.0, 1.0, 1.0, 1.0] and list(outs2[1]["info"]) == [0, 0, -2, 0]
    for i in (0, 2):
        for key in keep[i]:
            np.testing.assert_array_equal(outs2[i][key], keep[i][key])


def test_the_plan_refuses_before_any_device_work():
    md = D.DeviceOrder.model_desc(None, 1, 1, 1, 1, 0, 2)
    with pytest.raises(ValueError, match="nothing to differentiate"):
        D.BandedMultiGradPlan([None], [md], [np.zeros((1, 11))], [([], False)])
    with pytest.raises(ValueError, match="2 requests for 1 orders"):
        D.BandedMultiGradPlan([None], [None], [None], [([], True)] * 2)
    with pytest.raises(ValueError, match="solver must be 'banded' or 'auto'"):
        D.BandedMultiGradPlan([None], [md], [np.zeros((1, 11))], [([], True)], solver="dense")


@pytest.mark.parametrize("name", EB.CASES)
def test_bounds_and_kink_distances_of_the_cases(name):
    orders, models, em, P = EB.build(name)
    assert [EB.own_columns(em, i) for i in range(3)] == [list(c) for c in em._layout()[1]]
    bounds = EB.unit_bounds(orders, models, em, P)
    for i, (b, (lo, hi)) in enumerate(zip(bounds, EB.BOUNDS[name])):
        print(f"case {name} order {i} (N = {len(orders[i]['wave'])}): bounds {list(b)}")
        assert b.shape == (3,) and (b >= lo).all() and (b <= hi).all(), (name, i, b)
        assert (b <= EB.WINDOW).all()
    if name in ("A", "B"):
        assert min(len(o["wave"]) for o in orders) == 64 and min(int(b.min()) for b in bounds) > 64  # wider than an order
    else:
        longest = int(np.argmax([len(o["wave"]) for o in orders]))
        assert longest == 1 and bounds[1].max() < min(bounds[0].min(), bounds[2].min())  # the longest order is not the widest
    off = EB.kink_distance(orders, models, em, P)
    print(f"case {name}: the nearest local-kernel centre is {off:.4f} pixel from a kink")
    assert off >= 1e-3 and abs(off - EB.KINK[name]) <= 0.06 * EB.KINK[name]


def test_case_c_wide_differs_from_case_c_in_one_unit_only():
    orders, models, em, P = EB.build("C")
    _, _, em_w, P_w = EB.build("C-wide")
    j = em.labels.index("order1:global_cov:log_ls")
    assert em_w.labels == em.labels and (np.delete(P_w, j, axis=1) == np.delete(P, j, axis=1)).all()
    assert (P_w[[0, 2], j] == P[[0, 2], j]).all() and P_w[1, j] == np.log(40.0)
    bounds, wide = EB.unit_bounds(orders, models, em, P), EB.unit_bounds(orders, models, em_w, P_w)
    print(f"case C-wide: bounds of order 1 {list(wide[1])}")
    assert 470 <= wide[1][1] <= 490
    for i in range(3):
        keep = [0, 2] if i == 1 else [0, 1, 2]
        np.testing.assert_array_equal(wide[i][keep], bounds[i][keep])
    fits = D.banded_units(wide, [EB.WINDOW] * 3)
    assert [list(f) for f in fits] == [[True] * 3, [True, False, True], [True] * 3]
