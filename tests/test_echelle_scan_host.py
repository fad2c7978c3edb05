"""Host logic of the multi-order score scan (sf_local_scan_banded_multi_batch_md, sf_local_scan_mean, BandedMultiScanPlan and
EchelleModel.local_kernel_scan / propose_local_kernels): the candidate lists and h_cand_ptr, the output offsets, the routing
table, the peak picking per order through a stubbed scan, the refusals that name the order, and the C-ABI names.  No device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from starfish_amd import _device as D
from starfish_amd import _lib
from starfish_amd import _multi as M
from starfish_amd.models import EchelleModel
from starfish_amd.models._diagnostics import DEFAULT_SCAN_SIGMAS

import echelle_banded_cases as EB

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
NEW_NAMES = {"sf_local_scan_banded_multi_max_patch": 3, "sf_local_scan_banded_multi_workspace_bytes_md": 4,
             "sf_local_scan_banded_multi_batch_md": 12, "sf_local_scan_mean": 7}
EINVAL, FAKE = -1, 0x10000  # (a pointer that is not NULL; the calls below return before they read it)
WHO = "sf_local_scan_banded_multi_batch_md:"


def test_new_entry_points_are_declared_bound_and_exported():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "starfish_amd.h")).read()
    for name, nargs in NEW_NAMES.items():
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        declared = re.search(rf"^(?:size_t|int) {name}\s*\(([^;]*)\);", header, re.M)
        assert declared and declared.group(1).count(",") + 1 == nargs, name
    for name in ("local_kernel_scan", "local_kernel_scan_batch", "propose_local_kernels"):
        assert callable(getattr(EchelleModel, name, None)), name
    for name in ("local_scan_banded_multi", "BandedMultiScanPlan", "scan_routes", "scan_cand_ptr", "scan_out_offsets"):
        assert getattr(D, name) is getattr(M, name), name


def test_a_bad_segment_list_is_refused_by_name_before_anything_is_looked_at():
    lib = _lib.load()
    for segs, nseg in ((None, 3), (FAKE, 0), (FAKE, -1)):
        rc = lib.sf_local_scan_banded_multi_batch_md(C.cast(segs, C.POINTER(_lib.Segment)), nseg, None, FAKE, None, FAKE, FAKE, None, FAKE,
                                                     FAKE, 1 << 40, None)
        msg = lib.sf_last_error().decode()
        assert rc == EINVAL and msg.startswith(WHO) and "segment list" in msg, (nseg, msg)
        assert lib.sf_local_scan_banded_multi_workspace_bytes_md(C.cast(segs, C.POINTER(_lib.Segment)), nseg, None, None) == 0
        assert lib.sf_local_scan_banded_multi_max_patch(C.cast(segs, C.POINTER(_lib.Segment)), nseg, None) == EINVAL
    seg = (_lib.Segment * 1)(_lib.Segment(None, FAKE, 3, 0))
    md = _lib.ModelDesc()
    mds = (C.POINTER(_lib.ModelDesc) * 1)(C.pointer(md))
    rc = lib.sf_local_scan_banded_multi_batch_md(seg, 1, mds, FAKE, (C.c_int * 2)(0, 5), FAKE, FAKE, None, FAKE, FAKE, 1 << 40, None)
    msg = lib.sf_last_error().decode()
    assert rc == EINVAL and msg.startswith(WHO) and "segment 0" in msg, msg
    for args in ((0, 0, None, FAKE, FAKE, FAKE, None), (3, 5, None, FAKE, FAKE, FAKE, None), (3, 0, FAKE, FAKE, FAKE, FAKE, None),
                 (3, 5, FAKE, FAKE, FAKE, None, None)):
        assert lib.sf_local_scan_mean(*args) == EINVAL and lib.sf_last_error().decode().startswith("sf_local_scan_mean:"), args


def test_candidate_lists_and_cand_ptr():
    orders, models, em, P = EB.build("B")  # orders of 180, 64 and 256 pixels
    waves = [np.asarray(o["wave"], dtype=np.float64) for o in orders]
    # every order's own pixels x the default widths, width-major
    inputs = em._scan_inputs(None, None, None, "auto")
    assert [len(v[2]) for v in inputs] == [3 * 180, 3 * 64, 3 * 256]
    for (mus, sigmas, cand), w in zip(inputs, waves):
        np.testing.assert_array_equal(mus, w)
        np.testing.assert_array_equal(sigmas, DEFAULT_SCAN_SIGMAS)
        np.testing.assert_array_equal(cand[:, 0], np.tile(w, 3))
        np.testing.assert_array_equal(cand[:, 1], np.repeat(DEFAULT_SCAN_SIGMAS, len(w)))
    counts = [len(v[2]) for v in inputs]
    assert M.scan_cand_ptr(counts).tolist() == [0, 540, 732, 1500] and M.scan_cand_ptr(counts).dtype == np.int32
    # a list of centres per order, widths shared or per order
    mine = [waves[0][::7], waves[1][[3, 9]], waves[2][5:6]]
    inputs = em._scan_inputs(mine, (8.0, 30.0), None, "auto")
    assert [len(v[2]) for v in inputs] == [2 * len(mine[0]), 4, 2]
    np.testing.assert_array_equal(inputs[1][2], [(waves[1][3], 8.0), (waves[1][9], 8.0), (waves[1][3], 30.0), (waves[1][9], 30.0)])
    inputs = em._scan_inputs(mine, [(8.0,), (15.0, 30.0), (12.0,)], None, "auto")
    assert [v[1].tolist() for v in inputs] == [[8.0], [15.0, 30.0], [12.0]] and [len(v[2]) for v in inputs] == [len(mine[0]), 4, 1]
    # a wl_range that empties one order: its entry is None, the others keep the centres inside it
    lo, hi = waves[1][10], waves[2][19]
    inputs = em._scan_inputs(None, (15.0,), (lo, hi), "auto")
    assert inputs[0] is None
    np.testing.assert_array_equal(inputs[1][0], waves[1][10:])
    np.testing.assert_array_equal(inputs[2][0], waves[2][:20])
    with pytest.raises(ValueError, match="2 lists of centres for 3 orders"):
        em._scan_inputs(mine[:2], None, None, "auto")
    with pytest.raises(ValueError, match="2 lists of widths for 3 orders"):
        em._scan_inputs(None, [(8.0,), (15.0,)], None, "auto")
    with pytest.raises(ValueError, match="order 1: .*positive and finite"):
        em._scan_inputs([mine[0], [-1.0], mine[2]], None, None, "auto")
    with pytest.raises(ValueError, match="solver must be"):
        em._scan_inputs(None, None, None, "band")


def test_output_offsets_and_rounds():
    assert M.scan_out_offsets([3, 3, 3], [540, 192, 768]).tolist() == [0, 4860, 6588, 13500]
    assert M.scan_out_offsets([2, 5, 1], [7, 1, 65535]).tolist() == [0, 42, 57, 57 + 3 * 65535]
    assert M.scan_out_offsets([2], [4]).dtype == np.int64
    assert M.scan_out_offsets([65535, 65535], [65535, 65535])[-1] == 2 * 3 * 65535 * 65535  # (beyond 2^31)
    assert M.scan_rounds([3, 5]) == [[(0, 3, True), (0, 5, True)]]
    # a list longer than one call takes: every order stays in every call (one frame); a used-up list repeats its last candidate
    assert M.scan_rounds([3, 70000, 65535]) == [[(0, 3, True), (0, 65535, True), (0, 65535, True)],
                                                [(2, 3, False), (65535, 70000, True), (65534, 65535, False)]]
    assert M.scan_rounds([5, 2], step=2) == [[(0, 2, True), (0, 2, True)], [(2, 4, True), (1, 2, False)], [(4, 5, True), (1, 2, False)]]
    with pytest.raises(ValueError, match="at least one candidate per order"):
        M.scan_rounds([3, 0])


def test_the_routing_table():
    """banded / auto x the unit fits or not x the candidates fit or not, on made-up bounds: window 144, patch limit 145."""
    limit = 145
    narrow, wide = np.array([0, 31, 145]), np.array([12, 146])
    bounds = [np.array([100, 144, 145, 480]), np.array([10, 300])]
    # "banded": every order banded; a candidate beyond the limit or an order without a limit is an error naming the order
    assert M.scan_routes("banded", [narrow, narrow], [limit, limit]) == ["banded", "banded"]
    with pytest.raises(ValueError, match=r'order 1: a candidate reaches 146 pixels.*at most 145 pixels.*solver="auto"'):
        M.scan_routes("banded", [narrow, wide], [limit, limit])
    with pytest.raises(ValueError, match="order 0: .*does not take this order"):
        M.scan_routes("banded", [narrow, narrow], [0, limit])
    # "auto": an order with a candidate beyond the limit, or without a limit, goes dense as a whole
    assert M.scan_routes("auto", [narrow, wide], [limit, limit]) == ["auto", "dense"]
    assert M.scan_routes("auto", [narrow, narrow], [limit, 0]) == ["auto", "dense"]
    assert M.scan_routes("auto", [wide, narrow], [limit, 129]) == ["dense", "dense"]
    with pytest.raises(ValueError, match="solver must be"):
        M.scan_routes("dense", [narrow], [limit])
    # the units: a bound up to limit - 1 fits; the window of a dense order is -1 (nothing fits)
    for routes, windows in ((["auto", "auto"], [144, 144]), (["auto", "dense"], [144, -1])):
        assert [limit - 1 if r != "dense" else -1 for r in routes] == windows
        fits = M.banded_units(bounds, windows)
        assert fits[0].tolist() == [True, True, False, False]
        assert fits[1].tolist() == ([True, False] if windows[1] > 0 else [False, False])
        infos = [np.where(f, 0, D.INFO_BANDWIDTH) for f in fits]
        infos[0][1] = D.INFO_BANDWIDTH  # (the fill's probe flags a unit the host bound let through)
        rest = M.rerouted_units(fits, infos, "auto")
        assert rest[0].tolist() == [1, 2, 3] and rest[1].tolist() == ([1] if windows[1] > 0 else [0, 1])
        rest = M.rerouted_units(fits, infos, "banded")  # refused units stay refused
        assert rest[0].tolist() == [] and rest[1].tolist() == []
        infos[1][0] = D.INFO_INTERNAL  # the internal status goes dense under either solver
        assert M.rerouted_units(fits, infos, "banded")[1].tolist() == [0]


def test_the_mean_rule_on_the_host():
    rng = np.random.default_rng(3)
    quad, trace, fisher = rng.standard_normal((4, 6)) + 3, rng.standard_normal((4, 6)), rng.uniform(0.5, 2.0, (4, 6))
    fisher[:, 5] = 0.0  # no pixel in reach
    info = np.array([0, -1, 0, 0])
    z, amp, count = M.scan_mean_host(quad, trace, fisher, info)
    good = [0, 2, 3]
    U = 0.5 * (quad - trace)
    f = fisher[:, :5]
    want_z = ((U[0, :5] / np.sqrt(f[0]) + U[2, :5] / np.sqrt(f[2])) + U[3, :5] / np.sqrt(f[3])) / 3
    want_a = ((U[0, :5] / f[0] + U[2, :5] / f[2]) + U[3, :5] / f[3]) / 3
    assert count == 3 and len(good) == 3
    np.testing.assert_array_equal(z[:5], want_z)
    np.testing.assert_array_equal(amp[:5], want_a)
    assert np.isnan(z[5]) and np.isnan(amp[5])
    z, amp, count = M.scan_mean_host(quad, trace, fisher, np.full(4, -4))
    assert count == 0 and np.isnan(z).all() and np.isnan(amp).all()


def stubbed(em, means):
    """``em`` with the scan replaced by hand-made ``(z, amp, mus, sigmas)`` per order."""
    em._scan_means = lambda P, mus, sigmas, wl_range, solver: means
    return em


def test_propose_picks_per_order_through_a_stubbed_scan():
    orders, models, em, P = EB.build("A")  # 0, 1 and 2 local kernels... whatever each order can still take
    waves = [np.asarray(o["wave"], dtype=np.float64) for o in orders]
    sig = np.array([8.0, 15.0])
    means = []
    for i, w in enumerate(waves):
        z, amp = np.zeros((2, len(w))), np.full((2, len(w)), 1e-4)
        means.append([z, amp, w, sig])
    means[0][0][1, 20] = 9.0   # order 0: one peak at pixel 20, width 15
    means[1][0][0, 5] = 7.0    # order 1: two peaks far apart, the second stronger
    means[1][0][1, 100] = 8.0
    means[1][1][1, 100] = 2e-4
    means[2] = None            # order 2: skipped (no centre inside the range)
    got = stubbed(em, [None if v is None else tuple(v) for v in means]).propose_local_kernels(solver="auto")
    assert [len(v) for v in got] == [1, 2, 0]
    assert got[0] == [dict(mu=float(waves[0][20]), log_amp=float(np.log(1e-4)), log_sigma=float(np.log(15.0)))]
    assert [k["mu"] for k in got[1]] == [float(waves[1][5]), float(waves[1][100])]
    assert got[1][1]["log_amp"] == float(np.log(2e-4)) and got[1][0]["log_sigma"] == float(np.log(8.0))
    # max_kernels counts per order: each keeps its strongest
    one = em.propose_local_kernels(max_kernels=1, solver="auto")
    assert [len(v) for v in one] == [1, 1, 0] and one[1][0]["mu"] == float(waves[1][100])
    # None: as many as each order can still take -- order 1 made nearly full, four peaks far apart
    models[1]._local_kernels = lambda: [None] * (D.MAX_LOCAL - 2)
    for k in range(4):
        means[1][0][0, 5 + 30 * k] = 6.0 + 0.01 * k
    means[1][0][1, 100] = 0.0
    full = stubbed(em, [None if v is None else tuple(v) for v in means]).propose_local_kernels(solver="auto")
    assert [k["mu"] for k in full[1]] == [float(waves[1][65]), float(waves[1][95])] and len(full[0]) == 1
    assert len(em.propose_local_kernels(max_kernels=3, solver="auto")[1]) == 3
    nothing = em.propose_local_kernels(threshold=10.0, solver="auto")
    assert nothing == [[], [], []]


def test_refusals_name_the_order():
    orders, models, em, P = EB.build("A")
    models[1].solver = "auto"
    for call in (lambda: em.local_kernel_scan(), lambda: em.local_kernel_scan_batch(P), lambda: em.propose_local_kernels(),
                 lambda: em.propose_local_kernels(P=P, solver=None)):
        with pytest.raises(ValueError, match=r"order 1: solver=None runs the scan on the dense solver only, not solver='auto'"):
            call()
    models[1].solver = "dense"

    # no walker of P evaluates in an order: the device's (or the host's) count of that order is 0
    def run(P, inputs, solver, mean=False):
        assert mean
        return [(np.zeros(len(v[2])), np.zeros(len(v[2])), 3 if i != 2 else 0) for i, v in enumerate(inputs)], None

    em._scan_run = run
    with pytest.raises(ValueError, match="order 2: no walker of P evaluates"):
        em.propose_local_kernels(P=P, solver="auto")
    del em._scan_run
    with pytest.raises(ValueError, match="Param Vector does not match"):
        em._scan_run(P[:, :-1], em._scan_inputs(None, None, None, "dense"), "dense")
