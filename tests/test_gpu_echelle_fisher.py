"""sf_fisher_banded_multi_batch_md, sf_multi_fisher_reduce, BandedMultiFisherPlan and EchelleModel's Fisher information: the
Fisher matrices of all (order x walker) units in the mean-flux parameters from one sweep per unit and one launch sequence, and
their sum over the orders.

Inputs: tests/echelle_fisher_cases.py (cases A, B, C, C-wide of tests/echelle_banded_cases.py; D: 10 columns beside 8, two orders
carry zero rows; E: 17 rows, the second block of right-hand sides and the 128-pixel window).  The case builder asserts the row
counts and that no unit of A - E is refused or re-routed.

Bound on entry (a, b) of the summed matrix, from the np.longdouble references alone: the sum over the contributing orders of
FR.entry_bound(ref_i, banded=...) (tests/fisher_reference.py; N is the order's own length: the frame's further rows are identity
rows of the band with zero right-hand sides, which add exact zeros to every sum of the sweep, and an order's zero rows add exact
zeros to the Gram matrix) plus gamma(n_orders) sum_i |F_i| for the order sum.  Largest err / bound measured on an MI355X:
DESIGN.md, "Fisher information of an echelle model".  Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest

from gpu_helpers import oracle_order
from starfish_amd import _device as D
from starfish_amd import _lib, samplers

import echelle_fisher_cases as EF
import echelle_gradient_cases as EG
import fisher_reference as FR

pytestmark = pytest.mark.gpu

_CASES = {}
KEYS = ("lnl", "info", "fisher")


def case(name):
    """Model, walkers, packed rows and the device results every test of that case shares (made once, never written)."""
    if name not in _CASES:
        orders, models, em, P = EF.build(name)
        labels, cols, columns, sources = em._fisher_layout(solver="banded")
        packed = [m._pack(P[:, cols[i]], update_caches=False) for i, m in enumerate(models)]
        devs, mds, rows = ([p[k] for p in packed] for k in range(3))
        c = dict(orders=orders, models=models, em=em, P=P, labels=labels, cols=cols, columns=columns, sources=sources, devs=devs,
                 mds=mds, rows=rows, mean=em.mean_gradient_labels, refs={})
        c["plan"] = D.fisher_banded_multi(devs, mds, rows, columns, sync=False)
        c["out"] = c["plan"].collect()
        c["total"] = c["plan"].reduce(sources)
        c["plist"] = [[EF.oracle_params(m, P[b, cols[i]]) for b in range(len(P))] for i, m in enumerate(models)]
        if name in EF.ROWS:
            plan = c["plan"]
            assert tuple(len(v) for v in columns) == EF.COLUMNS[name]
            assert 1 + devs[0].m + plan.pmax == EF.ROWS[name]
            window = EF.WINDOWS[EF.ROWS[name]]
            assert plan._windows() == [window] * 3 and max(int(b.max()) for b in plan.bounds) <= window - 2
            assert plan.complete and plan.rerouted == 0 and all((o["info"] == 0).all() for o in c["out"])
        _CASES[name] = c
    return _CASES[name]


def ref_of(c, i, b):
    if (i, b) not in c["refs"]:
        c["refs"][i, b] = FR.reference(oracle_order(c["orders"][i]), c["plist"][i][b], c["models"][i].mean_gradient_labels)
    return c["refs"][i, b]


def index_of(c, i):
    """(labels, slots): the positions in the summed matrix of order i's columns, and their slots in its unit matrix."""
    pairs = [(j, slot) for j, src in enumerate(c["sources"]) for k, slot in src if k == i]
    return np.array([j for j, _ in pairs]), np.array([s for _, s in pairs])


def summed_reference(c, b, banded):
    """(F, bound) of walker b: the np.longdouble sum of the orders' references embedded by the sources, and the bound of
    the module docstring."""
    p, n = len(c["mean"]), len(c["orders"])
    F, bound, size = np.zeros((p, p), dtype=np.longdouble), np.zeros((p, p)), np.zeros((p, p))
    for i in range(n):
        ref = ref_of(c, i, b)
        la, sl = index_of(c, i)
        ix, sx = np.ix_(la, la), np.ix_(sl, sl)
        F[ix] += ref["Fld"][sx]
        bound[ix] += FR.entry_bound(ref, banded=banded)[0][sx]
        size[ix] += np.abs(ref["Fld"][sx]).astype(np.float64)
    return F, bound + EG.gamma(n) * size


def fraction(err, bound):
    """err / bound; where the bound is 0 -- entries between labels of different orders -- nothing but an exact 0 passes."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))


def cross_order_pairs(c):
    mean = c["mean"]
    return [(a, b) for a, ka in enumerate(mean) for b, kb in enumerate(mean)
            if ka.startswith("order") and kb.startswith("order") and ka.split(":")[0] != kb.split(":")[0]]


@pytest.mark.parametrize("name", EF.CASES)
def test_every_entry_of_the_sum_within_the_bound_of_the_longdouble_reference(name):
    """Largest err / bound measured on an MI355X: see DESIGN.md, "Fisher information of an echelle model"."""
    c = case(name)
    em, P, p = c["em"], c["P"], len(c["mean"])
    for solver in ("dense", "banded"):
        got, info, units = em.fisher_information_batch(P, return_info=True, return_orders=True, solver=solver)
        assert got.shape == (3, p, p) and (info == 0).all() and np.isfinite(got).all()
        assert [u.shape for u in units] == [(3, k, k) for k in EF.COLUMNS[name]]
        worst = 0.0
        for b in range(3):
            F, bound = summed_reference(c, b, solver == "banded")
            frac = fraction(np.abs(got[b] - F.astype(np.float64)), bound)
            worst = max(worst, frac.max())
            assert (frac <= 1.0).all(), (name, solver, b, frac.max(), np.unravel_index(frac.argmax(), frac.shape))
        # the guard against a wrong weight, on a unit: U^T U omitted lies far outside the agreement actually measured
        ref = ref_of(c, 0, 0)
        d = np.sqrt(np.diag(ref["F64"]))
        agree = (np.abs(units[0][0] - ref["F64"]) / np.outer(d, d)).max()
        wrong = FR.fisher_woodbury(ref["J"], ref["Bd"], ref["Y"], drop_uu=True)[0]
        off = (np.abs(wrong - ref["F64"]) / np.outer(d, d)).max()
        print(f"{name} {solver}: largest err / bound {worst:.3g}; order 0 walker 0: |device - float64 helper| / sqrt(F_ii F_jj) "
              f"{agree:.3g}, U^T U omitted {off:.3g} away")
        assert off > 10 * agree, (name, solver, off, agree)


@pytest.mark.parametrize("name", EF.CASES)
def test_structure_and_likelihood(name):
    c = case(name)
    em, P = c["em"], c["P"]
    cross = cross_order_pairs(c)
    own = [k - 5 for k in EF.COLUMNS[name]]  # (an order's columns but the five shared ones are its own labels)
    assert len(cross) == sum(own) ** 2 - sum(k * k for k in own)
    for solver in ("dense", "banded"):
        F, info = em.fisher_information_batch(P, return_info=True, solver=solver)
        lnl_g, _grad, info_g = em.log_likelihood_gradient_batch(P, return_info=True, solver=solver)
        if solver == "banded":
            lnl = c["total"][0]
            np.testing.assert_array_equal(F, c["total"][1])
        else:
            dense = [dev.fisher_mean(md, r, cols) for dev, md, r, cols in zip(c["devs"], c["mds"], c["rows"], c["columns"])]
            lnl = D.reduce_fisher_host(np.stack([o["lnl"] for o in dense]), np.stack([o["info"] for o in dense]),
                                       [o["fisher"] for o in dense], c["sources"])[0]
        print(f"{name} {solver}: lnl {lnl!r}, the gradient call's {lnl_g!r}")
        np.testing.assert_array_equal(info, info_g)
        np.testing.assert_array_equal(lnl, lnl_g)
        for b in range(3):
            assert np.array_equal(F[b], F[b].T) and (np.diag(F[b]) > 0).all()
            for a, k in cross:
                assert F[b, a, k] == 0.0 and not np.signbit(F[b, a, k])
            ref, bound = summed_reference(c, b, solver == "banded")
            d = np.sqrt(np.diag(ref).astype(np.float64))
            # F is positive semi-definite; an entrywise error E, |E| <= bound, moves an eigenvalue of D^-1 F D^-1 by at most
            # |D^-1 E D^-1|_2 <= the Frobenius norm of the normalised bound
            floor = -np.linalg.norm(bound / np.outer(d, d))
            low = np.linalg.eigvalsh(F[b] / np.outer(d, d))[0]
            print(f"{name} {solver} walker {b}: smallest eigenvalue of D^-1 F D^-1 {low:.3g} (floor {floor:.3g})")
            assert low >= floor


@pytest.mark.parametrize("name", EF.CASES)
def test_the_device_reduce_is_the_host_rule_and_units_agree_with_the_single_order_call(name):
    c = case(name)
    em, P = c["em"], c["P"]
    F, info, units = em.fisher_information_batch(P, return_info=True, return_orders=True, solver="banded")
    for u, out in zip(units, c["out"]):
        np.testing.assert_array_equal(u, out["fisher"])
    unit_lnl, unit_info = np.stack([o["lnl"] for o in c["out"]]), np.stack([o["info"] for o in c["out"]])
    host = D.reduce_fisher_host(unit_lnl, unit_info, units, c["sources"])
    for a, b in zip(c["total"], host):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(c["total"], EF.reduce_restated(unit_lnl, unit_info, units, c["sources"])):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(F, c["total"][1])
    np.testing.assert_array_equal(info, c["total"][2])
    np.testing.assert_array_equal(em.last_info, info)
    again = D.fisher_banded_multi(c["devs"], c["mds"], c["rows"], c["columns"], sync=False)
    for rep, out in zip(again.collect(), c["out"]):
        for key in KEYS:
            np.testing.assert_array_equal(rep[key], out[key], err_msg=f"a repeated call: {key}")
    for a, b in zip(again.reduce(c["sources"]), c["total"]):
        np.testing.assert_array_equal(a, b)
    # a unit against the same order's own call: another frame, another instantiation of the sweep -- both within the bound
    worst = 0.0
    for i, m in enumerate(c["models"]):
        own = m.fisher_information_batch(P[:, c["cols"][i]], solver="banded")
        assert own.shape == units[i].shape
        for b in range(3):
            bound = FR.entry_bound(ref_of(c, i, b), banded=True)[0]
            frac = np.abs(units[i][b] - own[b]) / (2 * bound)
            worst = max(worst, frac.max())
            assert (frac <= 1.0).all(), (name, i, b, frac.max())
            assert np.array_equal(units[i][b], units[i][b].T)
    print(f"{name}: largest |unit - the order's own call| / (2 bound) {worst:.3g}")


def test_zero_rows_leave_the_shorter_orders_blocks_alone():
    """Case D: orders 0 and 2 carry two zero rows behind their 8 columns; without order 1 the call has 11 rows and none."""
    c = case("D")
    pick = [0, 2]
    plan = D.fisher_banded_multi([c["devs"][i] for i in pick], [c["mds"][i] for i in pick], [c["rows"][i] for i in pick],
                                 [c["columns"][i] for i in pick], sync=False)
    alone = plan.collect()
    assert plan.pmax == 8 and c["plan"].pmax == 10 and plan.complete and plan.rerouted == 0
    worst = 0.0
    for i, out in zip(pick, alone):
        assert out["fisher"].shape == (3, 8, 8) and (out["info"] == 0).all()
        for b in range(3):
            bound = FR.entry_bound(ref_of(c, i, b), banded=True)[0]
            frac = np.abs(out["fisher"][b] - c["out"][i]["fisher"][b]) / (2 * bound)
            worst = max(worst, frac.max())
            assert (frac <= 1.0).all(), (i, b, frac.max())
    print(f"D: largest |with zero rows - without| / (2 bound) {worst:.3g}")
    # beyond a unit's own block the plan's buffer holds the zero rows' exact zeros
    raw = c["plan"].plan.fisher.cpu().numpy()
    assert raw.shape == (9, 10, 10) and (raw[0:3, 8:, :] == 0.0).all() and (raw[0:3, :, 8:] == 0.0).all()
    assert (raw[6:9, 8:, :] == 0.0).all() and (raw[6:9, :, 8:] == 0.0).all()


def test_a_unit_beyond_the_window_is_refused_under_banded_and_dense_under_auto():
    c = case("C")
    w = case("C-wide")
    em, P, sources = w["em"], w["P"], w["sources"]
    plan = w["plan"]
    assert [list(f) for f in plan.fits] == [[True] * 3, [True, False, True], [True] * 3] and not plan.complete
    assert plan.halfwidth == c["plan"].halfwidth  # (the group's largest bound is that of case C: same frame, same bits)
    out = w["out"]
    assert out[1]["info"][1] == D.INFO_BANDWIDTH and np.isneginf(out[1]["lnl"][1]) and np.isnan(out[1]["fisher"][1]).all()
    for i in range(3):
        keep = [0, 2] if i == 1 else [0, 1, 2]
        for key in KEYS:
            np.testing.assert_array_equal(out[i][key][keep], c["out"][i][key][keep], err_msg=f"banded order {i} {key}")
    lnl, F, info = w["total"]
    assert list(info) == [0, D.INFO_BANDWIDTH, 0] and np.isneginf(lnl[1]) and np.isnan(F[1]).all()
    np.testing.assert_array_equal(F[[0, 2]], c["total"][1][[0, 2]])
    np.testing.assert_array_equal(lnl[[0, 2]], c["total"][0][[0, 2]])
    got, ginfo = em.fisher_information_batch(P, return_info=True, solver="banded")
    np.testing.assert_array_equal(got, F)
    np.testing.assert_array_equal(ginfo, info)
    # "auto": that unit has the bits of the dense call on its row, every other unit those of case C; the sum is the host twin's
    plan = D.fisher_banded_multi(w["devs"], w["mds"], w["rows"], w["columns"], solver="auto", sync=False)
    out = plan.collect()
    assert plan.rerouted == 1 and all((o["info"] == 0).all() for o in out)
    dense = w["devs"][1].fisher_mean(w["mds"][1], w["rows"][1][1:2], w["columns"][1])
    for key in KEYS:
        np.testing.assert_array_equal(out[1][key][1], dense[key][0], err_msg=key)
    for i in range(3):
        keep = [0, 2] if i == 1 else [0, 1, 2]
        for key in KEYS:
            np.testing.assert_array_equal(out[i][key][keep], c["out"][i][key][keep], err_msg=f"auto order {i} {key}")
    got, ginfo, units = em.fisher_information_batch(P, return_info=True, return_orders=True, solver="auto")
    host = D.reduce_fisher_host(np.stack([o["lnl"] for o in out]), np.stack([o["info"] for o in out]), [o["fisher"] for o in out],
                                sources)
    np.testing.assert_array_equal(got, host[1])
    np.testing.assert_array_equal(got, plan.reduce(sources)[1])
    for u, o in zip(units, out):
        np.testing.assert_array_equal(u, o["fisher"])
    assert list(ginfo) == [0, 0, 0] and np.isfinite(got).all()
    np.testing.assert_array_equal(got[[0, 2]], c["total"][1][[0, 2]])


def c_call(c, halfwidth, requests=None, ld=None, stride=None, size_only=False):
    """sf_fisher_banded_multi_batch_md (or its size query) on the segments of the case's plan, with these arguments."""
    torch = D._torch()
    units = c["plan"].plan
    segs, nseg, _u0, n, models = units.calls[0]
    reqs = units._requests_array(list(range(nseg))) if requests is None else requests
    hw = (C.c_int * nseg)(*([halfwidth] * nseg))
    lib = units.lib
    nbytes = lib.sf_fisher_banded_multi_workspace_bytes_md(segs, nseg, models, reqs, hw)
    if size_only:
        return nbytes
    ld = units.stride if ld is None else ld
    stride = ld * ld if stride is None else stride
    with torch.cuda.device(units.dev):
        lnl, info = D.empty((n,), units.dev), D.empty((n,), units.dev, torch.int32)
        fisher = torch.full((n, max(stride, 1)), -7.0, dtype=torch.float64, device=units.dev)
        ws = D.workspace(max(nbytes, 1 << 20), units.dev)
        rc = lib.sf_fisher_banded_multi_batch_md(segs, nseg, models, reqs, hw, D.ptr(lnl), None, D.ptr(info), D.ptr(fisher), ld, stride,
                                                 D.ptr(ws), ws.numel(), D.stream_ptr(units.dev))
        _lib.check(rc, "sf_fisher_banded_multi_batch_md")
        return lnl.cpu().numpy(), info.cpu().numpy(), fisher.cpu().numpy()


def test_the_window_at_the_calls_row_count_and_the_other_refusals_of_the_c_call():
    """Case E has 17 rows: the window is 128, though every segment's own window of 1 + m rows is 144."""
    c = case("E")
    units = c["plan"].plan
    assert c_call(c, 128, size_only=True) > 0 and c_call(c, 129, size_only=True) == 0 and c_call(c, 144, size_only=True) == 0
    for hw in (129, 144):
        with pytest.raises(_lib.StarfishAMDError, match="sf_fisher_mean_batch"):
            c_call(c, hw)
    with pytest.raises(_lib.StarfishAMDError, match="sf_fisher_mean_batch"):
        c_call(c, 145)  # (beyond the segment's own window: the message of the frame check names it too)
    assert c_call(case("A"), 144, size_only=True) > 0  # 11 rows: the likelihood's window
    # the layout: a wider leading dimension and stride give the same blocks, and nothing is written beyond them
    H, p = c["plan"].halfwidth, units.stride
    lnl, info, F = c_call(c, H)
    np.testing.assert_array_equal(F.reshape(9, p, p), units.fisher.cpu().numpy())
    np.testing.assert_array_equal(lnl, units.quad[0].cpu().numpy())
    lnl2, info2, wide = c_call(c, H, ld=p + 3, stride=(p + 3) * (p + 3) + 5)
    np.testing.assert_array_equal(wide[:, :(p + 3) * (p + 3)].reshape(9, p + 3, p + 3)[:, :p, :p], F.reshape(9, p, p))
    assert (wide[:, (p + 3) * (p + 3):] == -7.0).all() and (wide[:, :(p + 3) * (p + 3)].reshape(9, p + 3, p + 3)[:, p:, :] == -7.0).all()
    np.testing.assert_array_equal(lnl2, lnl)
    # a half-width below the units' support flags them
    low = c_call(c, 16)
    assert (low[1] == D.INFO_BANDWIDTH).all() and np.isneginf(low[0]).all() and np.isnan(low[2].reshape(9, p, p)).all()
    # refusals before anything is enqueued
    for ld, stride, word in ((p - 1, None, "fisher_ld"), (p, p * p - 1, "fisher_stride")):
        with pytest.raises(_lib.StarfishAMDError, match=word):
            c_call(c, H, ld=ld, stride=stride)
    for change, word in ((dict(want_cov=1), "want_cov"), (dict(n_mean_slots=0), "no mean slot")):
        reqs = units._requests_array([0, 1, 2])
        for key, v in change.items():
            setattr(reqs[1], key, v)
        assert units.lib.sf_fisher_banded_multi_workspace_bytes_md(units.calls[0][0], 3, units.calls[0][4], reqs,
                                                                   (C.c_int * 3)(H, H, H)) == 0
        with pytest.raises(_lib.StarfishAMDError, match=f"segment 1.*{word}"):
            c_call(c, H, requests=reqs)


def test_failed_units_get_a_nan_matrix_and_leave_every_other_unit_alone():
    c = case("A")
    rows = [r.copy() for r in c["rows"]]
    rows[1][1, 0] = -1.0  # vsini of walker 1 in segment 1: status -2
    plan = D.fisher_banded_multi(c["devs"], c["mds"], rows, c["columns"], sync=False)
    out = plan.collect()
    assert list(out[1]["info"]) == [0, -2, 0] and np.isneginf(out[1]["lnl"][1]) and np.isnan(out[1]["fisher"][1]).all()
    for i in range(3):
        keep = [0, 2] if i == 1 else [0, 1, 2]
        for key in KEYS:
            np.testing.assert_array_equal(out[i][key][keep], c["out"][i][key][keep], err_msg=f"order {i} {key}")
    lnl, F, info = plan.reduce(c["sources"])
    assert list(info) == [0, -2, 0] and np.isneginf(lnl[1]) and np.isnan(F[1]).all()
    np.testing.assert_array_equal(F[[0, 2]], c["total"][1][[0, 2]])
    # through the model, on both solvers: a walker off the grid (-1) and one with a negative vsini (-2)
    em, P, labels = c["em"], c["P"], list(c["labels"])
    P2 = P.copy()
    P2[1, labels.index("T")] = 9000.0
    P2[2, labels.index("vsini")] = -1.0
    for solver in ("banded", "dense"):
        good = em.fisher_information_batch(P, solver=solver)
        F2, info2 = em.fisher_information_batch(P2, return_info=True, solver=solver)
        assert list(info2) == [0, -1, -2] and np.isnan(F2[1:]).all()
        np.testing.assert_array_equal(F2[0], good[0])


def test_the_reduce_kernel_on_made_up_units():
    """sf_multi_fisher_reduce alone: more pairs than one workgroup, a label without a source, labels of one, two and three
    orders, a failed unit, a source outside the unit block (not read: NaN), a leading dimension wider than the blocks."""
    torch = D._torch()
    lib = _lib.require_gpu()
    dev = D.device_of(None)
    rng = np.random.default_rng(5)
    nseg, W, ld = 3, 4, 16
    stride = ld * ld + 2
    ps = (16, 14, 15)
    fishers = []
    for p in ps:
        a = rng.standard_normal((W, p, p))
        fishers.append(a + a.transpose(0, 2, 1))
    raw = np.full((nseg * W, stride), 1e300)
    for i, f in enumerate(fishers):
        block = np.full((W, ld, ld), 1e300)
        block[:, :ps[i], :ps[i]] = f
        raw[i * W:(i + 1) * W, :ld * ld] = block.reshape(W, -1)
    lnl = rng.standard_normal((nseg, W))
    info = np.zeros((nseg, W), dtype=np.int32)
    info[2, 1] = -1
    sources = [[(0, k), (1, k), (2, k)] for k in range(5)] + [[(0, 5), (2, 6)], []]
    sources += [[(i, k)] for i in range(nseg) for k in range(5, ps[i]) if (i, k) not in ((0, 5), (2, 6))]
    assert len(sources) * (len(sources) + 1) // 2 > 256 > len(sources)

    def run(srcs):
        col_ptr, col_src = D.column_map_csr(srcs)
        n = len(srcs)
        with torch.cuda.device(dev):
            t = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (lnl.ravel(), info.ravel(), raw, col_ptr, col_src)]
            o_lnl, o_info = D.empty((W,), dev), D.empty((W,), dev, torch.int32)
            o_f = torch.full((W, n * n + 3), -7.0, dtype=torch.float64, device=dev)
            rc = lib.sf_multi_fisher_reduce(nseg, W, D.ptr(t[0]), D.ptr(t[1]), D.ptr(t[2]), ld, stride, D.ptr(t[3]), D.ptr(t[4]), n,
                                            D.ptr(o_lnl), D.ptr(o_f), n * n + 3, D.ptr(o_info), D.stream_ptr(dev))
            _lib.check(rc, "sf_multi_fisher_reduce")
            f = o_f.cpu().numpy()
            assert (f[:, n * n:] == -7.0).all()
            return o_lnl.cpu().numpy(), f[:, :n * n].reshape(W, n, n), o_info.cpu().numpy()

    got = run(sources)
    for a, b in zip(got, EF.reduce_restated(lnl, info, fishers, sources)):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(got, D.reduce_fisher_host(lnl, info, fishers, sources)):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(got, run(sources)):
        np.testing.assert_array_equal(a, b)
    assert list(got[2]) == [0, -1, 0, 0] and np.isnan(got[1][1]).all() and np.isfinite(got[1][[0, 2, 3]]).all()
    # a source outside the unit block: its entries are NaN, every other entry is what it was
    outside = [list(s) for s in sources]
    outside[5] = [(0, 5), (2, ld)]
    bad = run(outside)[1]
    touched = np.zeros((len(sources),) * 2, dtype=bool)
    for j, src in enumerate(sources):
        if any(i == 2 for i, _ in src):
            touched[5, j] = touched[j, 5] = True
    assert np.isnan(bad[0][touched]).all()
    np.testing.assert_array_equal(bad[0][~touched], got[1][0][~touched])
    with pytest.raises(_lib.StarfishAMDError, match="out_stride"):
        col_ptr, col_src = D.column_map_csr(sources)
        with torch.cuda.device(dev):
            t = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (lnl.ravel(), info.ravel(), raw, col_ptr, col_src)]
            o = D.empty((W, len(sources) ** 2), dev)
            rc = lib.sf_multi_fisher_reduce(nseg, W, D.ptr(t[0]), D.ptr(t[1]), D.ptr(t[2]), ld, stride, D.ptr(t[3]), D.ptr(t[4]),
                                            len(sources), D.ptr(o), D.ptr(o), len(sources) ** 2 - 1, D.ptr(t[1]), D.stream_ptr(dev))
            _lib.check(rc, "sf_multi_fisher_reduce")


def test_model_methods():
    c = case("A")
    _, _, em, P = EF.build("A")  # (a model of its own: its state is changed here)
    em.set_param_vector(P[0])
    for solver in (None, "banded", "auto"):
        F = em.fisher_information_batch(P, solver=solver)
        before = em.get_param_vector().copy()
        np.testing.assert_array_equal(em.fisher_information(solver=solver), F[0])
        np.testing.assert_array_equal(em.get_param_vector(), before)
    np.testing.assert_array_equal(em.fisher_information_batch(P, solver="banded"), c["total"][1])
    keep = ("vz", "vsini", "logg", "order0:log_scale", "order1:log_scale", "order2:log_scale")
    em.freeze([k for k in em.labels if k not in keep])
    assert em.mean_gradient_labels == keep == em.labels
    ref, bound = summed_reference(c, 0, True)
    ix = np.ix_(*[[c["mean"].index(k) for k in keep]] * 2)
    Fld = ref[ix]
    cond = np.linalg.cond(FR.normalised(Fld))
    print("condition number of the normalised block of", keep, cond)
    assert cond < 64.0  # (31.2 here; 15.5 and 33.2 for the same block of cases B and C)
    d = np.sqrt(np.diag(Fld).astype(np.float64))
    want = np.linalg.inv(Fld.astype(np.float64))
    # first order: |d(F^-1)| <= |F^-1| |dF| |F^-1|; in normalised form with |D^-1 dF D^-1| <= e entrywise and p x p matrices that
    # is at most p^2 cond^2 e on D cov D
    e = (bound[ix] / np.outer(d, d)).max()
    p = len(keep)
    for solver in (None, "banded"):
        cov = em.parameter_covariance(solver=solver)
        assert cov.shape == (p, p) and np.array_equal(cov, cov.T)
        err = (np.abs(cov - want) * np.outer(d, d)).max()
        print(f"parameter_covariance(solver={solver}): |D (cov - ref) D| {err:.3g}, allowed {p * p * cond**2 * e:.3g}; "
              f"sigma = {np.sqrt(np.diag(cov))}")
        assert err <= p * p * cond**2 * e
    start = samplers.gaussian_ball(em.get_param_vector(), cov, 16)
    assert np.asarray(start).shape == (16, p) and np.isfinite(start).all()
