"""The Fisher information of the mean-flux parameters on the device: sf_fisher_mean_batch (dense factor, F = Z^T Z) and
sf_fisher_banded_mean_batch (one sweep over [r; Y; J], F = G_JJ - U^T U) through DeviceOrder.fisher_mean and the SpectrumModel
methods.

Orders and walkers of tests/test_gpu_banded_gradient.py (make_order(seed=5), walker_ball(B=3, seed=3)):

    case          rows          row blocks
    N180          1 + 4 + 8     1     last 256-pixel block and last 16-row block both partial
    N256          13            1
    N330          13            1
    N180-Av       1 + 4 + 7     1
    N180-c6       1 + 4 + 12    2     six Chebyshev terms: 17 rows, one past the 16-row block
    N180-m17      1 + 17 + 8    2
    N330-narrow   1 + 24 + 8    3     make_order(m=24), log_ls = log 2: host bounds 60 .. 62, the 112-pixel window
    N512-narrow   1 + 24 + 8    3     the same at 32 block columns: the only case that takes the two half sweeps (nbr = 5 needs 30),
                                      with the call's own workspace for 33 rows; every other case runs one sweep per walker

No case may skip or fall back, which the case builder asserts.  Every entry of both calls is held to the reference-only bound of
tests/fisher_reference.py against the np.longdouble dense F; the dense call is the yardstick for the banded one and the largest
fraction of the bound is printed for both.  The Python calls return no flux (the dense C call has no such output), so the
agreement with loglike is checked on lnl and info for them; the banded C call's d_resid is asked for through _run_fisher and
held against loglike's residual."""
import numpy as np
import pytest

from starfish_amd import _device as D
from starfish_amd import _lib, synth

import fisher_reference as FR
from gpu_helpers import device_order, oracle_order, pack_rows
from test_fisher_host import wrong_weights
from test_gpu_mean_gradient import MEAN, columns
from test_gpu_model import close_lnl

pytestmark = pytest.mark.gpu

CASES = ["N180", "N256", "N330", "N180-Av", "N180-c6", "N180-m17", "N330-narrow", "N512-narrow"]
ROWS = {"N180": 13, "N256": 13, "N330": 13, "N180-Av": 12, "N180-c6": 17, "N180-m17": 26, "N330-narrow": 33, "N512-narrow": 33}


def twists(do, halfwidth, B):
    """Whether the band call of B walkers at this half-width takes two half sweeps per walker: the rule of sf_band_shape.h
    (sfb_twist_pays; tests/test_hostmath.py holds it) at the compute units of this device."""
    import torch

    ncu = torch.cuda.get_device_properties(do.dev).multi_processor_count
    nbr, nblk = max(3, (halfwidth + 31) // 16), (do.n + 15) // 16
    rounds1, rounds2 = -(-B // ncu), -(-2 * B // ncu)
    return nblk >= 6 * nbr and 0.5 * rounds2 + 0.12 * rounds1 < rounds1


_CASES = {}


def case(name):
    """Order, DeviceOrder, rows, the device results of both calls and (lazily, ``refs``) the references every test of that case
    shares: made once, never written."""
    if name not in _CASES:
        N = int(name[1:4])
        m = 17 if name.endswith("m17") else 24 if name.endswith("narrow") else 4
        o = synth.make_order(N=N, m=m, seed=5)
        oo = oracle_order(o)
        do = device_order(oo)
        P = synth.walker_ball(o, B=3, seed=3)
        plist = [synth.vector_to_oracle_params(p) for p in P]
        labels = MEAN
        if name.endswith("Av"):
            for p in plist:
                del p["vz"], p["vsini"]
                p["Av"] = 0.3
            labels = ("log_scale", "cheb:1", "cheb:2", "T", "logg", "Z", "Av")
        if name.endswith("c6"):
            for p in plist:
                p["cheb"] = [*p["cheb"], 0.004, -0.003, 0.002, -0.001]
            labels = ("vz", "vsini", "log_scale", *(f"cheb:{k}" for k in range(1, 7)), "T", "logg", "Z")
        if name.endswith("narrow"):
            for p in plist:
                p["global_cov"] = (p["global_cov"][0], float(np.log(2.0)))
        md, rows = pack_rows(do, plist)
        c = dict(N=N, m=m, o=o, oo=oo, do=do, P=P, plist=plist, md=md, rows=rows, labels=labels, slots=columns(do, md, labels), refs={})
        c["hw"] = do.halfwidth_bound(md, rows)
        p = len(labels)
        assert 1 + m + p == ROWS[name]
        # inside the window at this row count: nothing is refused, nothing goes to the dense call under "auto"
        assert do.fisher_banded_max_slots(int(c["hw"].max())) >= p, (c["hw"], p)
        if name.endswith("narrow"):
            assert c["hw"].min() >= 60 and c["hw"].max() <= 62 and do.fisher_banded_max_slots(112) >= p > do.fisher_banded_max_slots(113)
        assert twists(do, int(c["hw"].max()), 3) == (name == "N512-narrow"), (name, c["hw"])
        c["dense"] = do.fisher_mean(md, rows, c["slots"])
        c["banded"] = do.fisher_mean(md, rows, c["slots"], solver="banded")
        _CASES[name] = c
    return _CASES[name]


def ref_of(c, b):
    if b not in c["refs"]:
        c["refs"][b] = FR.reference(c["oo"], c["plist"][b], c["labels"])
    return c["refs"][b]


@pytest.mark.parametrize("name", CASES)
def test_every_entry_within_the_bound_of_the_longdouble_reference(name):
    """Largest err / bound measured on an MI355X: see DESIGN.md, "Fisher information in the mean-flux parameters"."""
    c = case(name)
    p = len(c["labels"])
    worst = {}
    for call in ("dense", "banded"):
        out = c[call]
        assert out["fisher"].shape == (3, p, p) and (out["info"] == 0).all() and np.isfinite(out["fisher"]).all()
        worst[call] = agree = 0.0
        for b in range(3):
            ref = ref_of(c, b)
            F = ref["Fld"].astype(np.float64)
            d = np.sqrt(np.diag(F))
            bound, _ = FR.entry_bound(ref, banded=call == "banded")
            frac = np.abs(out["fisher"][b] - F) / bound
            worst[call] = max(worst[call], frac.max())
            agree = max(agree, (np.abs(out["fisher"][b] - ref["F64"]) / np.outer(d, d)).max())
            assert (frac <= 1.0).all(), (name, call, b, frac.max(), np.unravel_index(frac.argmax(), frac.shape))
        print(f"{name} {call}: largest err / bound {worst[call]:.3g}; |device - float64 helper| / sqrt(F_ii F_jj) {agree:.3g}")
        # the guard against a wrong weight: the variants of the host test lie outside the agreement actually measured
        if "cheb:2" in c["labels"] and c["labels"] == MEAN:
            ref = ref_of(c, 0)
            d = np.sqrt(np.diag(ref["F64"]))
            for what, wrong in wrong_weights(c["oo"], c["plist"][0], ref).items():
                off = (np.abs(wrong - ref["F64"]) / np.outer(d, d)).max()
                print(f"    {what}: {off:.3g} of sqrt(F_ii F_jj) away")
                assert off > 10 * agree, (what, off, agree)
    print(f"{name}: largest err / bound: banded {worst['banded']:.3g}, dense {worst['dense']:.3g}")


@pytest.mark.parametrize("name", CASES)
def test_structure_and_likelihood(name):
    c = case(name)
    do, md, rows = c["do"], c["md"], c["rows"]
    like = do.loglike(md, rows, want_resid=True)
    band = do.loglike(md, rows, solver="banded")
    # d_resid of the banded C call (model minus data), which fisher_mean does not ask for: the same bits with it
    p, W = len(c["slots"]), int(c["hw"].max())
    raw = do._run_fisher("fisher_banded_mean_batch", md, rows, (W, (_lib.C.c_int * p)(*c["slots"]), p), p, True,
                         lambda units: do.fisher_banded_mean_workspace_bytes(md, units, W, p), None)
    for key in ("lnl", "fisher", "info"):
        np.testing.assert_array_equal(raw[key], c["banded"][key], err_msg=key)
    flux = like["resid"] + c["oo"].flux[None, :]
    assert raw["resid"].shape == (3, c["N"])
    np.testing.assert_allclose(raw["resid"] + c["oo"].flux[None, :], flux, rtol=0, atol=1e-12 * np.abs(flux).max())
    assert (like["info"] == 0).all() and (band["info"] == 0).all()
    np.testing.assert_array_equal(c["dense"]["lnl"], like["lnl"])  # sf_loglike_batch's bits
    for call in ("dense", "banded"):
        out = c[call]
        for b in range(3):
            F = out["fisher"][b]
            assert close_lnl(out["lnl"][b], like["lnl"][b]) and close_lnl(out["lnl"][b], band["lnl"][b])
            assert np.array_equal(F, F.T) and (np.diag(F) > 0).all()
            ref = ref_of(c, b)
            d = np.sqrt(np.diag(ref["Fld"]).astype(np.float64))
            bound, _ = FR.entry_bound(ref, banded=call == "banded")
            # F is positive semi-definite; an entrywise error E, |E| <= bound, moves an eigenvalue of D^-1 F D^-1 by at most
            # |D^-1 E D^-1|_2 <= the Frobenius norm of the normalised bound
            floor = -np.linalg.norm(bound / np.outer(d, d))
            low = np.linalg.eigvalsh(F / np.outer(d, d))[0]
            print(f"{name} {call} walker {b}: smallest eigenvalue of D^-1 F D^-1 {low:.3g} (floor {floor:.3g})")
            assert low >= floor


@pytest.mark.parametrize("name", CASES)
def test_repeated_and_chunked_calls_give_the_same_bits_and_slot_subsets_agree_within_the_bound(name):
    c = case(name)
    do, md, rows, slots = c["do"], c["md"], c["rows"], c["slots"]
    for solver in ("dense", "banded"):
        for other in (do.fisher_mean(md, rows, slots, solver=solver), do.fisher_mean(md, rows, slots, solver=solver, max_chunk=1)):
            for key in ("lnl", "fisher", "info"):
                np.testing.assert_array_equal(other[key], c[solver][key], err_msg=f"{solver} {key}")
        for pick in (list(range(len(slots)))[::-2], [len(slots) - 1], [0]):  # (another row count: rounding, not bits)
            sub = do.fisher_mean(md, rows, [slots[j] for j in pick], solver=solver)
            assert sub["fisher"].shape == (3, len(pick), len(pick)) and (sub["info"] == 0).all()
            for b in range(3):
                ref = ref_of(c, b)
                bound, _ = FR.entry_bound(ref, banded=solver == "banded")
                ix = np.ix_(pick, pick)
                assert (np.abs(sub["fisher"][b] - ref["Fld"].astype(np.float64)[ix]) <= bound[ix]).all(), (solver, pick, b)
                assert np.array_equal(sub["fisher"][b], sub["fisher"][b].T)


def test_auto_takes_the_banded_call_where_it_fits():
    c = case("N256")
    auto = c["do"].fisher_mean(c["md"], c["rows"], c["slots"], solver="auto")
    for key in ("lnl", "fisher", "info"):
        np.testing.assert_array_equal(auto[key], c["banded"][key], err_msg=key)
    assert not np.array_equal(c["banded"]["fisher"], c["dense"]["fisher"])  # (another solve: rounding, not bits)


def test_failed_walkers_get_nan_matrices_and_leave_the_others_alone():
    c = case("N256")
    do, md, slots = c["do"], c["md"], c["slots"]
    rows = c["rows"].copy()
    rows[1, 0] = -1.0
    rows[2, 6] = 1e5
    for solver in ("dense", "banded"):
        out = do.fisher_mean(md, rows, slots, solver=solver)
        assert list(out["info"]) == [0, -2, -1] and np.isneginf(out["lnl"][1:]).all()
        assert np.isnan(out["fisher"][1:]).all()
        for key in ("fisher", "lnl"):
            np.testing.assert_array_equal(out[key][0], c[solver][key][0])
    # data without pixel noise and log_scale 18: the dense factorisation finds the matrix not positive definite
    o = dict(c["o"])
    o["sigma"] = np.zeros(c["N"])
    oo = oracle_order(o)
    dq = device_order(oo)
    plist = [dict(p) for p in c["plist"]]
    md2, good = pack_rows(dq, plist)
    plist[1]["log_scale"] = 18.0
    md2, mixed = pack_rows(dq, plist)
    clean = dq.fisher_mean(md2, good, slots)
    out = dq.fisher_mean(md2, mixed, slots)
    print("info of the mixed batch (dense)", out["info"])
    assert out["info"][1] > 0 and out["lnl"][1] == -np.inf and np.isnan(out["fisher"][1]).all()
    assert (out["info"][[0, 2]] == 0).all()
    np.testing.assert_array_equal(out["fisher"][[0, 2]], clean["fisher"][[0, 2]])
    band = dq.fisher_mean(md2, mixed, slots, solver="banded")  # (the band solver factorises Bd, not C: it may take the walker)
    print("info of the mixed batch (banded)", band["info"])
    for b in range(3):
        assert np.isnan(band["fisher"][b]).all() == (band["info"][b] != 0)
    np.testing.assert_array_equal(band["fisher"][[0, 2]], dq.fisher_mean(md2, good, slots, solver="banded")["fisher"][[0, 2]])


def test_a_walker_wider_than_the_half_width_is_flagged_and_auto_sends_it_to_the_dense_call():
    c = case("N256")
    do, slots = c["do"], c["slots"]
    plist = [dict(p) for p in c["plist"]]
    plist[1]["global_cov"] = (plist[1]["global_cov"][0], float(np.log(14.0)))
    md, rows = pack_rows(do, plist)
    hw, window = do.halfwidth_bound(md, rows), do.banded_window_halfwidth()
    print("half-width bounds", hw, "window", window)
    assert hw[1] > window and hw[0] <= window and hw[2] <= window
    out = do.fisher_mean(md, rows, slots, solver="banded")
    assert out["info"].tolist() == [0, D.INFO_BANDWIDTH, 0] and out["lnl"][1] == -np.inf and np.isnan(out["fisher"][1]).all()
    for key in ("fisher", "lnl"):
        np.testing.assert_array_equal(out[key][[0, 2]], c["banded"][key][[0, 2]])
    auto = do.fisher_mean(md, rows, slots, solver="auto")
    dense = do.fisher_mean(md, rows, slots)
    assert (auto["info"] == 0).all()
    for key in ("fisher", "lnl"):
        np.testing.assert_array_equal(auto[key][1], dense[key][1])
        np.testing.assert_array_equal(auto[key][[0, 2]], c["banded"][key][[0, 2]])
    # the C-ABI: a half-width below a walker's support flags it
    h = (_lib.C.c_int * len(slots))(*slots)
    low = do._run_fisher("fisher_banded_mean_batch", c["md"], c["rows"], (16, h, len(slots)), len(slots), False,
                         lambda units: do.fisher_banded_mean_workspace_bytes(c["md"], units, 16, len(slots)), None)
    assert (low["info"] == D.INFO_BANDWIDTH).all() and np.isneginf(low["lnl"]).all() and np.isnan(low["fisher"]).all()


@pytest.mark.parametrize("name", ["N180-m17", "N330-narrow"])
def test_a_half_width_past_the_window_at_this_row_count_raises_under_banded(name):
    """m = 17 with 8 columns is 26 rows (window 128), m = 24 is 33 rows (window 112): the walkers of the wide default kernel
    (bounds 115 .. 119) fit the likelihood's window of 1 + m rows but, for m = 24, not the one of the Fisher call's rows."""
    c = case(name)
    do, md, slots = c["do"], c["md"], c["slots"]
    p = len(slots)
    limit = max(w for w in range(0, 160, 16) if do.fisher_banded_max_slots(w) >= p)
    assert limit == (128 if name == "N180-m17" else 112) and do.fisher_banded_max_slots(limit + 1) < p
    assert do.fisher_banded_mean_workspace_bytes(md, 3, limit + 1, p) == 0 < do.fisher_banded_mean_workspace_bytes(md, 3, limit, p)
    h = (_lib.C.c_int * p)(*slots)
    with pytest.raises(_lib.StarfishAMDError, match="sf_fisher_mean_batch"):
        do._run_fisher("fisher_banded_mean_batch", md, c["rows"], (limit + 1, h, p), p, False, lambda units: 1 << 20, None)
    if name == "N330-narrow":  # the wide walkers through the Python layer
        plist = [dict(q) for q in c["plist"]]
        for q, vec in zip(plist, c["P"]):
            q["global_cov"] = synth.vector_to_oracle_params(vec)["global_cov"]
        md2, rows = pack_rows(do, plist)
        hw = do.halfwidth_bound(md2, rows)
        print("half-width bounds of the wide walkers", hw, "window of the likelihood", do.banded_window_halfwidth())
        assert (hw > 112).all() and (hw <= do.banded_window_halfwidth()).all()
        with pytest.raises(_lib.StarfishAMDError, match="sf_fisher_mean_batch"):
            do.fisher_mean(md2, rows, slots, solver="banded")
        auto = do.fisher_mean(md2, rows, slots, solver="auto")
        dense = do.fisher_mean(md2, rows, slots)
        for key in ("fisher", "lnl", "info"):
            np.testing.assert_array_equal(auto[key], dense[key], err_msg=key)


def test_slot_checks_that_need_a_context():
    c = case("N256")
    do, md, rows = c["do"], c["md"], c["rows"]
    for solver in ("dense", "banded"):
        for bad, word in (([2, 1, 2], "listed twice"), ([2, 4], "not a differentiable mean parameter"),
                          ([2, 6 + do.P + md.n_cheb], "not a differentiable mean parameter"),
                          (list(range(17)), "nslots=17")):
            with pytest.raises(_lib.StarfishAMDError, match=word):
                do.fisher_mean(md, rows, bad, solver=solver)
        with pytest.raises(ValueError, match="no column"):
            do.fisher_mean(md, rows, [], solver=solver)
    assert do.fisher_mean_workspace_bytes(md, 3, 8) > 0 and do.fisher_mean_workspace_bytes(md, 3, 17) == 0
    assert do.fisher_banded_mean_workspace_bytes(md, 3, 119, 8) > 0 and do.fisher_banded_mean_workspace_bytes(md, 3, 119, 0) == 0


def test_model_methods():
    c = case("N256")
    model = synth.build_model(c["o"])
    dev, md, rows = model._pack(c["P"], update_caches=False)
    cols = columns(dev, md, MEAN)
    assert model.mean_gradient_labels == MEAN
    for solver in (None, "banded", "auto"):
        raw = dev.fisher_mean(md, rows, cols, solver=solver or "dense")
        F, info = model.fisher_information_batch(c["P"], return_info=True, solver=solver)
        np.testing.assert_array_equal(F, raw["fisher"])
        assert (info == 0).all()
        model.set_param_vector(c["P"][0])
        np.testing.assert_array_equal(model.fisher_information(solver=solver), F[0])
    # the inverse: only vz, vsini and logg thawed -- the subset the data separate (the whole matrix is singular to 1e-12)
    model.freeze([k for k in model.labels if k not in ("vz", "vsini", "logg")])
    assert model.mean_gradient_labels == ("vz", "vsini", "logg")
    ref = ref_of(c, 0)
    ix = np.ix_(*[[MEAN.index(k) for k in ("vz", "vsini", "logg")]] * 2)
    Fld = ref["Fld"][ix]
    cond = np.linalg.cond(FR.normalised(Fld))
    print("condition number of the normalised (vz, vsini, logg) block", cond)
    assert cond < 4.0  # (measured: 1.4 here, N = 256; 1.6 .. 2.0 for the block at N = 180 and 330, m = 4 .. 24)
    bound, _ = FR.entry_bound(ref, banded=True)
    d = np.sqrt(np.diag(Fld).astype(np.float64))
    want = np.linalg.inv(Fld.astype(np.float64))
    # first order: |d(F^-1)| <= |F^-1| |dF| |F^-1|; in normalised form with |D^-1 dF D^-1| <= e entrywise and 3 x 3 matrices
    # that is at most 9 cond^2 e on D cov D
    e = (bound[ix] / np.outer(d, d)).max()
    for solver in (None, "banded"):
        cov = model.parameter_covariance(solver=solver)
        assert cov.shape == (3, 3) and np.array_equal(cov, cov.T)
        err = (np.abs(cov - want) * np.outer(d, d)).max()
        print(f"parameter_covariance(solver={solver}): |D (cov - ref) D| {err:.3g}, allowed {9 * cond**2 * e:.3g}; "
              f"sigma(vz, vsini, logg) = {np.sqrt(np.diag(cov))}")
        assert err <= 9 * cond**2 * e
