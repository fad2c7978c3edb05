"""sf_local_scan_banded_multi_batch_md, sf_local_scan_mean, BandedMultiScanPlan and EchelleModel's local kernel scan: the score
scan for new local kernels of all (order x walker) units from one launch sequence on the band + Woodbury solver.

Inputs: cases A, B, C and C-wide of tests/echelle_banded_cases.py (orders of 64 / 130 / 180, 180 / 64 / 256 and 130 / 330 / 64
pixels, m = 2 and 4, 0 - 3 local kernels, three walkers; a 64-pixel order in a 330-row frame, the longest order not the widest).
Candidates per order: those of tests/test_gpu_local_scan.py (every pixel x 8 / 15 / 30 km/s, two centres between pixels, one
clipped at the edge, one with no pixel in reach), the first extra centre moved to pixel N - 10 on an order shorter than 71 pixels.
The case builder asserts from host code alone: every patch <= 145 pixels, the call's limit; every unit of A - C fits the window
(no reroute); the three orders' candidate counts differ.

Bound: tests/test_gpu_banded_local_scan.py's ``bounds`` (its banded column), from np.longdouble references alone, with N the
order's own length -- the frame's further rows are identity rows of the band with zero right-hand sides, which add exact zeros
to every sum of the sweeps, and a shorter order's Sigma, Vs and alpha are read with its own n.  Against the single-order banded
call: the sum of the two calls' bounds.  sf_local_scan_mean against the host formula on the same triples: gamma_B mean|v| per
entry (B - 1 additions and the division; the quotients themselves are correctly rounded on both sides).  Largest err / bound
measured on an MI355X: DESIGN.md, "Score scan of an echelle model".  Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest

from oracle import sf_oracle as O
from starfish_amd import _device as D
from starfish_amd import _lib, synth
from starfish_amd.models import EchelleModel

import banded_derivatives as BD
import echelle_banded_cases as EB
import echelle_fisher_cases as EF
import echelle_gradient_cases as EG
import local_scan_reference as LS
import test_gpu_banded_local_scan as SINGLE
from gpu_helpers import oracle_order
from per_order_cases import PER, ball, per_order_models
from test_gpu_local_scan import SIGMAS, candidates
from test_gpu_model import close_lnl

pytestmark = pytest.mark.gpu

KEYS = ("quad", "trace", "fisher")
ALL = KEYS + ("lnl", "info")
LIMIT = 145  # sf_band_max_halfwidth(1 + m) + 1 for m <= 15
U = 2.0 ** -53


def candidates_for(wave):
    """tests/test_gpu_local_scan.py's candidates and subset for an order of any length: the first extra centre sits at pixel 70, or
    at N - 10 on an order shorter than 71 pixels; the subset keeps the pixels the order has."""
    wave = np.asarray(wave, dtype=np.float64)
    N = len(wave)
    step = wave[1] - wave[0]
    k = 70 if N > 70 else N - 10
    cand = [(w, s) for s in SIGMAS for w in wave]
    extra = [(wave[k] + 0.3 * step, 15.0), (wave[N // 2] + 0.5 * (wave[N // 2 + 1] - wave[N // 2]), 15.0), (wave[0] - 12 * step, 15.0),
             (wave[0] - 400 * step, 15.0)]
    pixels = sorted(p for p in set(range(0, N, 7)) | set(range(62, 67)) | set(range(126, 131)) | {0, 1, 2, N - 3, N - 2, N - 1} if p < N)
    subset = [s * N + j for s in range(3) for j in pixels] + [3 * N + e for e in range(len(extra))]
    cand = np.array(cand + extra)
    if N > 131:
        ref, ref_subset = candidates(wave)
        assert np.array_equal(cand, ref) and np.array_equal(subset, ref_subset)
    return cand, np.array(subset)


_CASES = {}


def case(name):
    """Model, walkers, packed rows, candidates and the device results every test of that case shares (made once, never written)."""
    if name in _CASES:
        return _CASES[name]
    orders, models, em, P = EB.build(name)
    labels, cols = em._layout()
    packed = [m._pack(P[:, cols[i]], update_caches=False) for i, m in enumerate(models)]
    devs, mds, rows = ([p[k] for p in packed] for k in range(3))
    both = [candidates_for(o["wave"]) for o in orders]
    cands, subsets = [b[0] for b in both], [b[1] for b in both]
    c = dict(orders=orders, models=models, em=em, P=P, cols=cols, devs=devs, mds=mds, rows=rows, cands=cands, subsets=subsets)
    # from host code alone: the patches, the window, the counts
    assert len({len(v) for v in cands}) == 3
    for o, dev, md, r, cand in zip(orders, devs, mds, rows, cands):
        lo, hi = D.local_scan_patches(o["wave"], cand)
        assert (hi - lo + 1).max() <= LIMIT and (hi - lo + 1)[-1] == 0 and dev.local_scan_banded_max_patch(md) == LIMIT
        if name != "C-wide":
            assert (dev.halfwidth_bound(md, r) <= LIMIT - 1).all()
    if name == "C-wide":
        hw = devs[1].halfwidth_bound(mds[1], rows[1])
        assert hw[1] > LIMIT - 1 and hw[0] <= LIMIT - 1 and hw[2] <= LIMIT - 1
    c["plan"] = D.local_scan_banded_multi(devs, mds, rows, cands, sync=False)
    c["out"] = c["plan"].collect()
    if name != "C-wide":
        assert c["plan"].rerouted == 0 and all((o["info"] == 0).all() for o in c["out"]) and len(c["plan"].plan.calls) == 1
        c["single"] = [dev.local_scan(md, r, cand, solver="banded") for dev, md, r, cand in zip(devs, mds, rows, cands)]
    c["sub"] = {}
    _CASES[name] = c
    return c


def sub_case(c, i):
    """Order i of the case in the shape tests/test_gpu_banded_local_scan.py's ``bounds`` takes.  Made once."""
    if i not in c["sub"]:
        o, dev, md, rows = c["orders"][i], c["devs"][i], c["mds"][i], c["rows"][i]
        oo = oracle_order(o)
        N = len(o["wave"])
        plist = [EF.oracle_params(c["models"][i], c["P"][b, c["cols"][i]]) for b in range(len(c["P"]))]
        s = dict(N=N, o=o, oo=oo, do=dev, m=int(dev.m), plist=plist, cand=c["cands"][i], subset=c["subsets"][i])
        s["resid"] = dev.apply(md, rows, "Cinv", want_flux=True)["flux"] - oo.flux[None, :]
        s["C64"] = [O.forward_model(oo, p)[1] + O.JITTER * np.eye(N) for p in plist]
        c["sub"][i] = s
    return c["sub"][i]


def triples(out):
    return np.stack([out[key] for key in KEYS], axis=-1)


@pytest.mark.parametrize("name", EB.CASES)
def test_every_unit_within_the_banded_bound_of_the_longdouble_reference(name):
    """Largest err / bound measured on an MI355X: see DESIGN.md, "Score scan of an echelle model"."""
    c = case(name)
    worst = dict.fromkeys(KEYS, 0.0)
    agree, off, missed = 0.0, 0.0, []
    for i in range(3):
        s = sub_case(c, i)
        wave = np.asarray(s["o"]["wave"])
        for b in range(3):
            ref_b = SINGLE.bounds(s, b)
            if i == 0 and b == 0:  # the guard's wrong reference: W without Vs Vs^T
                Sigma = np.linalg.inv(BD.pieces(s["oo"], s["plist"][b])["Bd"])
            for q, row in ref_b["rows"].items():
                got = [c["out"][i][key][b, q] for key in KEYS]
                if row is None:
                    assert got == [0.0, 0.0, 0.0], (name, i, b, q, got)
                    continue
                for k, key in enumerate(KEYS):
                    err = abs(got[k] - row["ref"][k])
                    worst[key] = max(worst[key], err / row["banded"][k])
                    if not (err <= row["banded"][k] and abs(got[k] - row["ref64"][k]) <= 1e-6 * row["size"][k]):
                        missed.append((name, i, b, q, key, got[k], row["ref"][k], row["banded"][k], row["ref64"][k]))
                if i == 0 and b == 0:
                    wrong = LS.three(Sigma, ref_b["alpha64"], wave, *s["cand"][q])
                    agree = max(agree, abs(got[1] - row["ref64"][1]) / row["size"][1])
                    off = max(off, abs(wrong[1] - row["ref64"][1]) / row["size"][1])
    print(f"{name}: largest err / bound " + ", ".join(f"{key} {v:.3g}" for key, v in worst.items())
          + f"; order 0 walker 0: |device - float64 reference| / size of the trace {agree:.3g}, Vs Vs^T dropped {off:.3g} away")
    assert not missed, missed[:5]
    assert off > 10 * agree, (name, off, agree)


@pytest.mark.parametrize("name", EB.CASES)
def test_against_the_single_order_banded_call(name):
    c = case(name)
    worst = dict.fromkeys(KEYS, 0.0)
    for i in range(3):
        s, got, one = sub_case(c, i), c["out"][i], c["single"][i]
        np.testing.assert_array_equal(got["info"], one["info"])
        for b in range(3):
            assert close_lnl(got["lnl"][b], one["lnl"][b]), (name, i, b, got["lnl"][b], one["lnl"][b])
            for q, row in SINGLE.bounds(s, b)["rows"].items():
                for k, key in enumerate(KEYS):
                    if row is None:
                        assert got[key][b, q] == 0.0 and one[key][b, q] == 0.0
                        continue
                    err = abs(got[key][b, q] - one[key][b, q])
                    worst[key] = max(worst[key], err / (2 * row["banded"][k]))
                    assert err <= 2 * row["banded"][k], (name, i, b, q, key, got[key][b, q], one[key][b, q])
        for key in KEYS:  # every candidate, not only the subset: finite, and exactly +0 with no pixel in reach
            assert got[key].shape == (3, len(c["cands"][i])) and np.isfinite(got[key]).all(), (name, i, key)
            assert (got[key][:, -1] == 0.0).all() and not np.signbit(got[key][:, -1]).any(), (name, i, key)
            scale = np.abs(one[key]).max()
            assert np.abs(got[key] - one[key]).max() <= 1e-8 * scale, (name, i, key)
    print(f"{name}: largest |multi - single| / (sum of the two bounds) " + ", ".join(f"{key} {v:.3g}" for key, v in worst.items()))


@pytest.mark.parametrize("name", ["A", "C"])
def test_same_bits_repeated_cut_and_with_another_orders_list_shortened(name):
    c = case(name)
    devs, mds, rows, cands, out = c["devs"], c["mds"], c["rows"], c["cands"], c["out"]
    again = D.local_scan_banded_multi(devs, mds, rows, cands)
    cut = D.local_scan_banded_multi(devs, mds, rows, cands, max_units=2, sync=False)
    assert len(cut.plan.calls) == 5 and [len(p) for p in cut.plan.pieces] == [1, 2, 1, 1, 1]  # (orders cut inside and across)
    cut = cut.collect()
    shorter = [cands[0], cands[1][5:22], cands[2]]
    short = D.local_scan_banded_multi(devs, mds, rows, shorter)
    for i in range(3):
        for key in ALL:
            np.testing.assert_array_equal(again[i][key], out[i][key], err_msg=f"repeated {i} {key}")
            np.testing.assert_array_equal(cut[i][key], out[i][key], err_msg=f"cut {i} {key}")
            want = out[i][key][:, 5:22] if i == 1 and key in KEYS else out[i][key]
            np.testing.assert_array_equal(short[i][key], want, err_msg=f"shortened {i} {key}")


def raw_arguments(c):
    """The one C call of the case's plan: (lib, units, call, h_cand_ptr, the length of d_out in doubles)."""
    units = c["plan"].plan
    call = units.calls[0]
    return units.lib, units, call, units._cand_ptr(0, call.orders), int(units.offsets[0][-1])


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_poisoned_layout_every_triple_is_written_and_nothing_outside(name):
    """The segments' slices are contiguous by contract (segment i starts at 3 sum_{j<i} B_j ncand_j), so the guard words stand
    before the first and behind the last; every slice is read at its documented offset and compared with that order's own
    single-order call -- a wrong offset for unequal ncand_i moves a slice onto its neighbour's numbers or onto the sentinel."""
    import torch

    c = case(name)
    lib, units, call, cand_ptr, total = raw_arguments(c)
    guard, sentinel = 96, -7.25
    sizes, counts = units.sizes, units.counts[0]
    offs = D.scan_out_offsets(sizes, counts)
    assert total == offs[-1] == 3 * sum(3 * len(v) for v in c["cands"]) and len(set(counts)) == 3
    with torch.cuda.device(units.dev):
        buf = torch.full((total + 2 * guard,), sentinel, dtype=torch.float64, device=units.dev)
        lnl = torch.full((9 + 2,), sentinel, dtype=torch.float64, device=units.dev)
        info = torch.full((9 + 2,), 77, dtype=torch.int32, device=units.dev)
        rc = lib.sf_local_scan_banded_multi_batch_md(call.segs, call.nseg, call.models, D.ptr(units.d_cand[0]), cand_ptr,
                                                     D.ptr(buf[guard:]), D.ptr(lnl[1:]), None, D.ptr(info[1:]), D.ptr(units.ws),
                                                     units.ws.numel(), D.stream_ptr(units.dev))
        _lib.check(rc, "sf_local_scan_banded_multi_batch_md")
        host, lnl, info = buf.cpu().numpy(), lnl.cpu().numpy(), info.cpu().numpy()
    assert (host[:guard] == sentinel).all() and (host[-guard:] == sentinel).all()
    assert lnl[0] == sentinel and lnl[-1] == sentinel and info[0] == 77 and info[-1] == 77 and (info[1:-1] == 0).all()
    body = host[guard:-guard]
    assert not (body == sentinel).any()
    for i in range(3):
        got = body[offs[i]:offs[i + 1]].reshape(sizes[i], counts[i], 3)
        np.testing.assert_array_equal(got, triples(c["out"][i]), err_msg=f"order {i}")  # (the plan reads the same layout)
        one = triples(c["single"][i])
        assert np.abs(got - one).max(axis=(0, 1)).tolist() <= (1e-8 * np.abs(one).max(axis=(0, 1))).tolist(), (name, i)
        np.testing.assert_array_equal(lnl[1 + 3 * i:4 + 3 * i], c["out"][i]["lnl"])


def test_c_wide_a_unit_beyond_the_window_and_a_candidate_beyond_the_limit():
    c = case("C-wide")
    devs, mds, rows, cands, out = c["devs"], c["mds"], c["rows"], c["cands"], c["out"]
    # "banded": walker 1 of order 1 is refused; its other orders and the other walkers are finite
    assert out[1]["info"].tolist() == [0, D.INFO_BANDWIDTH, 0] and out[1]["lnl"][1] == -np.inf
    for i in range(3):
        for key in KEYS:
            bad = np.isnan(out[i][key])
            assert bad[1].all() == (i == 1) and not bad[[0, 2]].any(), (i, key)
        if i != 1:
            assert (out[i]["info"] == 0).all() and np.isfinite(out[i]["lnl"]).all()
    # "auto": that unit has the dense scan's bits, every other unit the banded plan's
    auto = D.local_scan_banded_multi(devs, mds, rows, cands, solver="auto", sync=False)
    got = auto.collect()
    assert auto.rerouted == 1
    dense = devs[1].local_scan(mds[1], rows[1][1:2], cands[1])
    for key in ALL:
        np.testing.assert_array_equal(got[1][key][1:2], dense[key], err_msg=key)
        for i in range(3):
            keep = [0, 2] if i == 1 else [0, 1, 2]
            np.testing.assert_array_equal(got[i][key][keep], out[i][key][keep], err_msg=f"{i} {key}")
    # a 40 km/s width whose patch exceeds 145 pixels on the 330-pixel order
    wide = np.vstack([cands[1][::9], [(c["orders"][1]["wave"][165], 40.0)]])
    lo, hi = D.local_scan_patches(c["orders"][1]["wave"], wide[-1:])
    assert LIMIT < hi[0] - lo[0] + 1 <= D.LOCAL_SCAN_MAX_PATCH
    with pytest.raises(ValueError, match=r'order 1: a candidate reaches \d+ pixels.*at most 145 pixels'):
        D.local_scan_banded_multi(devs, mds, rows, [cands[0], wide, cands[2]], solver="banded")
    plan = D.local_scan_banded_multi(devs, mds, rows, [cands[0], wide, cands[2]], solver="auto", sync=False)
    assert plan.routes == ["auto", "dense", "auto"] and plan.on_device == [0, 2]
    got = plan.collect()
    dense = devs[1].local_scan(mds[1], rows[1], wide)
    for key in ALL:
        np.testing.assert_array_equal(got[1][key], dense[key], err_msg=key)
    assert np.isfinite(got[1]["fisher"][:, -1]).all() and (got[1]["info"] == 0).all()
    for i in (0, 2):  # (another frame without the 330-pixel order: to rounding)
        for key in KEYS:
            assert np.abs(got[i][key] - out[i][key]).max() <= 1e-8 * np.abs(out[i][key]).max(), (i, key)
    em = c["em"]
    mus = [None, [c["orders"][1]["wave"][165]], None]
    with pytest.raises(ValueError, match=r"order 1: candidate mu=.*reaches \d+ pixels.*at most 145 pixels"):
        em.local_kernel_scan_batch(c["P"], mus=[o["wave"][::9] if m is None else m for o, m in zip(c["orders"], mus)],
                                   sigmas=(15.0, 40.0), solver="banded")


def test_the_mean_on_the_device_against_the_host_formula():
    import torch

    c = case("A")
    units = c["plan"].plan
    lib, i = units.lib, 2
    t = units._triples(i)[0]
    B, ncand = int(t.shape[0]), int(t.shape[1])
    host = t.cpu().numpy()
    assert (host[:, -1, 2] == 0).all()  # (no pixel in reach: fisher == 0)
    gamma = B * U / (1 - B * U)
    for codes in ([0, 0, 0], [0, -1, 0], [3, 0, -4], [-1, -4, 2]):
        with torch.cuda.device(units.dev):
            info = torch.tensor(codes, dtype=torch.int32, device=units.dev)
            mean = torch.full((ncand + 1, 2), -7.25, dtype=torch.float64, device=units.dev)
            count = torch.full((3,), 77, dtype=torch.int32, device=units.dev)
            for _ in range(2):  # (a repeated call: the same bits)
                rc = lib.sf_local_scan_mean(B, ncand, D.ptr(t), D.ptr(info), D.ptr(mean), D.ptr(count[1:]), D.stream_ptr(units.dev))
                _lib.check(rc, "sf_local_scan_mean")
                got, n = mean.cpu().numpy(), count.cpu().numpy()
                if _ == 0:
                    first = got.copy()
            np.testing.assert_array_equal(got, first)
        z, amp, used = D.scan_mean_host(host[:, :, 0], host[:, :, 1], host[:, :, 2], np.array(codes))
        good = [b for b, code in enumerate(codes) if code == 0]
        assert n.tolist() == [77, len(good), 77] and used == len(good)
        assert (got[-1] == -7.25).all()  # (nothing behind the last candidate)
        if not good:
            assert np.isnan(got[:-1]).all() and np.isnan(z).all()
            continue
        assert np.isnan(got[-2]).all() and np.isnan(z[-1]) and np.isnan(amp[-1])  # fisher == 0
        score = 0.5 * (host[good, :-1, 0] - host[good, :-1, 1])
        for col, want, v in ((0, z, score / np.sqrt(host[good, :-1, 2])), (1, amp, score / host[good, :-1, 2])):
            bound = gamma * np.abs(v).mean(axis=0)
            err = np.abs(got[:-2, col] - want[:-1])
            assert np.isfinite(got[:-2, col]).all() and (err <= bound).all(), (codes, col, (err / bound).max())
            assert (np.abs(got[:-2, col] - v.mean(axis=0)) <= bound).all(), (codes, col)
    # the plan's read-out per order: device means, the host rule on the collected triples beside them
    means = c["plan"].mean()
    for i, (z, amp, used) in enumerate(means):
        o = c["out"][i]
        hz, ha, hn = D.scan_mean_host(o["quad"], o["trace"], o["fisher"], o["info"])
        assert used == hn == 3 and z.shape == (len(c["cands"][i]),)
        np.testing.assert_array_equal(z, hz)  # (the same operations in the same order)
        np.testing.assert_array_equal(amp, ha)
    # an order with a refused unit is averaged on the host, over the walkers that evaluate there
    w = case("C-wide")
    means = w["plan"].mean()
    assert [m[2] for m in means] == [3, 2, 3]
    o = w["out"][1]
    hz, _, _ = D.scan_mean_host(o["quad"][[0, 2]], o["trace"][[0, 2]], o["fisher"][[0, 2]], np.zeros(2, dtype=np.int32))
    np.testing.assert_array_equal(means[1][0], hz)


def test_the_model_methods_hand_the_plan_on_and_leave_the_model_alone():
    c = case("A")
    em, P, models, cols = c["em"], c["P"], c["models"], c["cols"]
    before = em.get_param_vector().copy()
    mus = [np.concatenate([o["wave"][::5], [o["wave"][0] - 400 * (o["wave"][1] - o["wave"][0])]]) for o in c["orders"]]
    # solver=None: the loop over the orders' dense scans, bit for bit
    res, info, codes = em.local_kernel_scan_batch(P, mus=mus, sigmas=SIGMAS, return_info=True, return_orders=True)
    assert (info == 0).all() and codes.shape == (3, 3) and (codes == 0).all()
    for i, m in enumerate(models):
        want = m.local_kernel_scan_batch(P[:, cols[i]], mus=mus[i], sigmas=SIGMAS)
        assert set(res[i]) == set(want) == {"score", "information", "z", "amp", "quad", "trace"}
        for key in want:
            assert res[i][key].shape == (3, 3, len(mus[i]))
            np.testing.assert_array_equal(res[i][key], want[key], err_msg=f"{i} {key}")
        assert (res[i]["information"][..., -1] == 0).all() and np.isnan(res[i]["z"][..., -1]).all()
    # "banded" / "auto": the plan's numbers
    cands = [np.array([(mu, s) for s in SIGMAS for mu in mm]) for mm in mus]
    raw = D.local_scan_banded_multi(c["devs"], c["mds"], c["rows"], cands)
    for solver in ("banded", "auto"):
        got = em.local_kernel_scan_batch(P, mus=mus, sigmas=SIGMAS, solver=solver)
        for i in range(3):
            for key, dkey in (("quad", "quad"), ("trace", "trace"), ("information", "fisher")):
                np.testing.assert_array_equal(got[i][key], raw[i][dkey].reshape(3, 3, len(mus[i])), err_msg=f"{solver} {i} {key}")
    # the current state is row 0 of the batch call on get_param_vector(); a range that empties an order skips it
    own = em.local_kernel_scan(sigmas=SIGMAS, solver="auto")
    batch = em.local_kernel_scan_batch(em.get_param_vector()[None, :], sigmas=SIGMAS, solver="auto")
    for i in range(3):
        for key in own[i]:
            assert own[i][key].shape == (3, len(c["orders"][i]["wave"]))
            np.testing.assert_array_equal(own[i][key], batch[i][key][0], err_msg=f"{i} {key}")
    lo, hi = c["orders"][1]["wave"][10], c["orders"][2]["wave"][19]
    part = em.local_kernel_scan(sigmas=(15.0,), wl_range=(lo, hi), solver="auto")
    assert part[0] is None and part[1]["z"].shape == (1, 120) and part[2]["z"].shape == (1, 20)
    np.testing.assert_array_equal(part[1]["quad"][0], own[1]["quad"][1, 10:])
    with pytest.raises(ValueError, match="solver must be"):
        em.local_kernel_scan(solver="band")
    np.testing.assert_array_equal(em.get_param_vector(), before)


def test_a_line_injected_into_one_order_is_proposed_there_and_nowhere_else():
    """Case B with a Gaussian bump of 5 sigma_noise and 15 km/s added to the data of order 0 at pixel 113 (22 pixels from the
    nearest of its local kernels).  The oracle's z at that centre and width is 18.3, checked here to exceed 4 x the threshold of
    4 (the factor this test states); without the line the oracle's z stays below 2 everywhere in that order."""
    FACTOR, THRESHOLD, PIX, WIDTH = 4.0, 4.0, 113, 15.0
    n_local, sizes, m, _ = EG.CASES["B"]
    orders, models = per_order_models(n_local, sizes=list(sizes), m=m, seed0=100)
    plain = EchelleModel.from_orders(models, per_order=PER)
    w = np.asarray(orders[0]["wave"])
    line = 5.0 * np.median(orders[0]["sigma"]) * np.exp(-0.5 * (O.C_KMS * (w - w[PIX]) / w[PIX] / WIDTH) ** 2)
    with_line = [dict(orders[0], flux=orders[0]["flux"] + line), orders[1], orders[2]]
    _, injected = per_order_models(n_local, sizes=list(sizes), m=m, seed0=100)
    p0 = dict(synth.centre_params(orders[0]))  # (order 0 as per_order_models builds it, on the data with the line)
    p0["local_cov"] = [dict(mu=float(w[(k + 1) * len(w) // (n_local[0] + 1)]), log_amp=-8.0 - 0.1 * k, log_sigma=float(np.log(12.0)))
                       for k in range(n_local[0])]
    p0.update(cheb=[0.01, -0.02], log_scale=0.0, global_cov=dict(log_amp=-9.0, log_ls=float(np.log(10.0))))
    injected[0] = synth.build_model(with_line[0], params=p0)
    em = EchelleModel.from_orders(injected, per_order=PER)
    assert em.labels == plain.labels
    np.testing.assert_array_equal(em.get_param_vector(), plain.get_param_vector())
    # the reference z on the CPU, from the oracle alone
    z_ref = {}
    for tag, o in (("line", with_line[0]), ("plain", orders[0])):
        oo = oracle_order(o)
        p = EF.oracle_params(models[0], models[0].get_param_vector())
        flux, cov = O.forward_model(oo, p)[:2]
        W = LS.cinv(cov + O.JITTER * np.eye(len(w)), np.float64)
        alpha = W @ (flux - oo.flux)
        q, t, f = LS.three(W, alpha, w, w[PIX], WIDTH)
        z_ref[tag] = 0.5 * (q - t) / np.sqrt(f)
    print("oracle z at the line", z_ref)
    assert z_ref["line"] >= FACTOR * THRESHOLD and z_ref["plain"] < THRESHOLD / 2
    l0 = em.orders[0].log_likelihood()
    got = em.propose_local_kernels(threshold=THRESHOLD, sigmas=SIGMAS, solver="auto")
    base = plain.propose_local_kernels(threshold=THRESHOLD, sigmas=SIGMAS, solver="auto")
    print("proposed in order 0:", got[0], "without the line:", base[0])
    reach = WIDTH / O.C_KMS * w[PIX]  # one width, in the units of the wavelengths
    assert base[0] == [] and len(got[0]) == 1 and abs(got[0][0]["mu"] - w[PIX]) <= reach
    assert got[0][0]["log_sigma"] == np.log(15.0)
    assert got[1] == base[1] and got[2] == base[2]  # the two other orders are not changed by the injection
    own = em.orders[0].propose_local_kernels(threshold=THRESHOLD, sigmas=SIGMAS, solver="auto")
    assert own[0]["mu"] == got[0][0]["mu"] and abs(own[0]["log_amp"] - got[0][0]["log_amp"]) <= 1e-9
    # with walkers: the means over the walkers, from the device
    P = ball(em, 3, seed=1)
    avg = em.propose_local_kernels(threshold=THRESHOLD, sigmas=SIGMAS, P=P, solver="auto", max_kernels=2)
    assert len(avg[0]) >= 1 and min(abs(k["mu"] - w[PIX]) for k in avg[0]) <= reach and all(len(v) <= 2 for v in avg)
    assert em.orders[0].log_likelihood() == l0


def test_every_refusal_names_the_call_and_enqueues_nothing():
    import torch

    c = case("A")
    lib, units, call, cand_ptr, total = raw_arguments(c)
    need = lib.sf_local_scan_banded_multi_workspace_bytes_md(call.segs, call.nseg, call.models, cand_ptr)
    assert 0 < need <= units.ws.numel() and lib.sf_local_scan_banded_multi_max_patch(call.segs, call.nseg, call.models) == LIMIT
    ptr3 = lambda *v: (C.c_int * 4)(*v)  # noqa: E731
    n0, n1, n2 = units.counts[0]
    oo = oracle_order(c["orders"][1])
    perm = np.random.default_rng(12).permutation(len(oo.wave))
    shuffled = D.DeviceOrder(oo.wave[perm], oo.flux[perm], oo.sigma[perm], oo.min_dv_wave, oo.bulk_fluxes, oo.grid_points,
                             oo.variances, oo.lengthscales, oo.v11, oo.w_hat)
    with torch.cuda.device(units.dev):
        out = torch.full((total,), 77.0, dtype=torch.float64, device=units.dev)
        lnl = torch.full((9,), 77.0, dtype=torch.float64, device=units.dev)
        info = torch.full((9,), 77, dtype=torch.int32, device=units.dev)
        bad_segs = (_lib.Segment * 3)(*[call.segs[k] for k in range(3)])
        bad_segs[1] = _lib.Segment(shuffled.ctx, call.segs[1].d_params, 3, 0)
        big = (_lib.Segment * 3)(*[call.segs[k] for k in range(3)])
        big[2] = _lib.Segment(call.segs[2].ctx, call.segs[2].d_params, 65536, 0)
        none = (_lib.Segment * 3)(*[call.segs[k] for k in range(3)])
        none[0] = _lib.Segment(None, call.segs[0].d_params, 3, 0)

        def run(segs=call.segs, nseg=call.nseg, models=call.models, cand=units.d_cand[0], cptr=cand_ptr, o=out, l=lnl, i=info,
                work=units.ws, nbytes=units.ws.numel()):
            rc = lib.sf_local_scan_banded_multi_batch_md(segs, nseg, models, D.ptr(cand), cptr, D.ptr(o), D.ptr(l), None, D.ptr(i),
                                                         D.ptr(work), nbytes, D.stream_ptr(units.dev))
            size = lib.sf_local_scan_banded_multi_workspace_bytes_md(segs, nseg, models, cptr)
            return rc, lib.sf_last_error().decode(), size

        sized = [(dict(nseg=0), "segment list"), (dict(models=None), "segment list"), (dict(segs=none), "segment 0"),
                 (dict(segs=bad_segs), "segment 1: the wavelength grid is not monotonic"), (dict(segs=big), "segment 2: B=65536"),
                 (dict(cptr=None), "h_cand_ptr"), (dict(cptr=ptr3(-1, n0, n0 + n1, n0 + n1 + n2)), "segment 0"),
                 (dict(cptr=ptr3(0, n0, n0, n0 + n2)), "segment 1: 0 candidates"),
                 (dict(cptr=ptr3(0, n0, n0 - 1, n0 + n2)), "segment 1: -1 candidates"),
                 (dict(cptr=ptr3(0, n0, n0 + n1, n0 + n1 + 65536)), "segment 2: 65536 candidates")]
        for kw, word in sized:
            rc, said, size = run(**kw)
            assert rc == -1 and said.startswith("sf_local_scan_banded_multi_batch_md:") and word in said and size == 0, (kw, rc, said)
        for kw in (dict(cand=None), dict(o=None), dict(l=None), dict(i=None), dict(work=None)):
            rc, said, size = run(**kw)
            assert rc == -1 and said.startswith("sf_local_scan_banded_multi_batch_md:") and "required" in said and size == need, (kw, said)
        rc, said, _ = run(nbytes=need - 1)
        assert rc == -2 and said.startswith("sf_local_scan_banded_multi_batch_md:") and "workspace too small" in said, said
        assert lib.sf_local_scan_banded_multi_max_patch(bad_segs, 3, call.models) == 0
        assert lib.sf_local_scan_banded_multi_max_patch(none, 3, call.models) == -1
        torch.cuda.synchronize()
        assert (out == 77.0).all() and (lnl == 77.0).all() and (info == 77).all()
        rc, said, _ = run(nbytes=need)
        torch.cuda.synchronize()
        assert rc == 0 and not (out == 77.0).any() and (info == 0).all(), (rc, said)
        np.testing.assert_array_equal(lnl.cpu().numpy(), np.concatenate([o["lnl"] for o in c["out"]]))
