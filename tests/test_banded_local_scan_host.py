"""The score scan on the band solver without a device: the new C-ABI names, what sf_local_scan_banded_batch refuses before it
looks at a context, the window's half-width per emulator rank that its patch limit is made of (through the host driver of
tests/test_hostmath.py, which exposes sf_band_shape.h), the routing of DeviceOrder.local_scan and what the SpectrumModel methods
refuse and hand to the device layer (tests/stand_in.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from starfish_amd import _device as D
from starfish_amd import _lib
from starfish_amd.models import SpectrumModel

from stand_in import StandIn, model_on_a_stand_in, state_of
from test_hostmath import driver, run  # noqa: F401  (the fixture that builds the stand-alone driver)

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
NEW_NAMES = {"sf_local_scan_banded_max_patch": 2, "sf_local_scan_banded_workspace_bytes": 4, "sf_local_scan_banded_batch": 12}
EINVAL, FAKE = -1, 0x10000  # (a pointer that is not NULL; the calls below return before they read it)
WHO = "sf_local_scan_banded_batch:"


def test_new_entry_points_are_declared_bound_and_exported():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "starfish_amd.h")).read()
    for name, nargs in NEW_NAMES.items():
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        declared = re.search(rf"^(?:size_t|int) {name}\s*\(([^;]*)\);", header, re.M)
        assert declared and declared.group(1).count(",") + 1 == nargs, name
    for name in ("local_scan", "local_scan_banded_max_patch", "local_scan_banded_workspace_bytes"):
        assert callable(getattr(D.DeviceOrder, name, None)), name
    import inspect

    for name in ("local_kernel_scan", "local_kernel_scan_batch", "propose_local_kernels"):
        assert inspect.signature(getattr(SpectrumModel, name)).parameters["solver"].default is None, name
    assert inspect.signature(D.DeviceOrder.local_scan).parameters["solver"].default == "dense"


def model_desc(has_global=0, n_local=0):
    md = _lib.ModelDesc()
    md.has_global, md.n_local = has_global, n_local
    return md


@pytest.mark.parametrize("kw,word", [(dict(B=0), "B=0"), (dict(B=-2), "B=-2"), (dict(B=65536), "B=65536"), (dict(ncand=0), "ncand=0"),
                                     (dict(ncand=-1), "ncand=-1"), (dict(ncand=65536), "ncand=65536")])
def test_the_counts_are_refused_before_the_context_is_looked_at(kw, word):
    lib = _lib.load()
    a = dict(dict(B=3, ncand=5), **kw)
    rc = lib.sf_local_scan_banded_batch(None, C.byref(model_desc()), a["B"], FAKE, FAKE, a["ncand"], FAKE, None, None, FAKE, 1 << 40, None)
    msg = lib.sf_last_error().decode()
    assert rc == EINVAL and msg.startswith(WHO) and word in msg, (kw, msg)
    assert lib.sf_local_scan_banded_workspace_bytes(None, C.byref(model_desc()), a["B"], a["ncand"]) == 0


def test_with_good_counts_the_missing_context_is_what_is_refused_whatever_kernels_the_model_has():
    lib = _lib.load()
    for kernels in ((0, 0), (1, 0), (1, 1), (0, 2)):
        rc = lib.sf_local_scan_banded_batch(None, C.byref(model_desc(*kernels)), 3, FAKE, FAKE, 5, FAKE, None, None, FAKE, 1 << 40, None)
        assert rc == EINVAL and lib.sf_last_error().decode() == WHO + " bad context / model descriptor", kernels
        assert lib.sf_local_scan_banded_workspace_bytes(None, C.byref(model_desc(*kernels)), 3, 5) == 0
        assert lib.sf_local_scan_banded_max_patch(None, C.byref(model_desc(*kernels))) == EINVAL
    assert lib.sf_local_scan_banded_workspace_bytes(None, None, 3, 5) == 0


def test_the_patch_limit_per_emulator_rank_is_the_windows_half_width_plus_one(driver):  # noqa: F811
    """sf_local_scan_banded_max_patch is sf_band_max_halfwidth(1 + m) + 1: 145 pixels up to m = 15, 129 up to 31, 113 beyond, none
    from 1 + m = 49 rows on; whatever it is, such a patch spans at most three 64-blocks beyond its first (the reach of the tiles)."""
    rc, err, v = run(driver, "band", 16, 50, 256)
    assert rc == 0, err
    maxhw = v["maxhw"].astype(int)  # (nrhs = 1 .. 50)
    for m in range(1, 50):
        wmax = int(maxhw[m])  # nrhs = 1 + m
        want = 144 if m <= 15 else 128 if m <= 31 else 112 if m <= 47 else -1
        assert wmax == want, (m, wmax)
        limit = wmax + 1
        assert limit <= D.LOCAL_SCAN_MAX_PATCH and (limit + 62) // 64 <= 3
    header = open(os.path.join(ROOT, "include", "starfish_amd.h")).read()
    assert "wmax = 144 / 128 / 112" in header


def test_routing_needs_no_device():
    for bad in ("band", "Dense", None, 1):
        with pytest.raises(ValueError, match="solver must be"):
            D.check_solver(bad)
    with pytest.raises(ValueError, match="solver must be"):
        D.local_scan_route("dense", [10], 145)  # (the dense call is not routed)
    pixels = np.array([0, 31, 145])
    assert D.local_scan_route("auto", pixels, 145) == "auto" and D.local_scan_route("banded", pixels, 145) == "banded"
    assert D.local_scan_route("auto", pixels, 129) == "dense"  # one candidate too wide: the whole call goes dense
    assert D.local_scan_route("banded", pixels, 129) == "banded"  # (the device marks it NaN)
    assert D.local_scan_route("auto", pixels, 0) == "dense" and D.local_scan_route("auto", [0], 0) == "dense"
    with pytest.raises(ValueError, match='does not take this order.*solver="dense" or "auto"'):
        D.local_scan_route("banded", pixels, 0)


class FakeOrder:
    """DeviceOrder.local_scan's routing on a grid of 2 km/s pixels: the calls it would make, recorded."""
    local_scan = D.DeviceOrder.local_scan

    def __init__(self, limit, hw):
        self.wave = 5000.0 * np.exp(np.arange(400) * (2.0 / D.C_KMS))
        self._keep, self.limit, self.hw, self.calls = [self.wave], limit, np.asarray(hw), []

    def local_scan_banded_max_patch(self, md):
        return self.limit

    local_scan_workspace_bytes = local_scan_banded_workspace_bytes = None

    def _host_rows_and_bound(self, md, params):
        return np.asarray(params), self.hw

    def _local_scan_call(self, name, md, params, cand, max_chunk, workspace_bytes):
        B, n = len(params), len(cand)
        self.calls.append((name, B, n))
        flag = 1.0 if name == "local_scan_batch" else 2.0
        info = np.zeros(B, dtype=np.int32)
        return dict(quad=np.full((B, n), flag), trace=np.full((B, n), flag), fisher=np.full((B, n), flag), lnl=np.full(B, flag), info=info)


def test_auto_goes_dense_for_a_wide_candidate_and_sends_the_walkers_that_do_not_fit_there():
    rows = np.zeros((3, 4))
    do = FakeOrder(145, [10, 200, 144])
    narrow = [(do.wave[200], 15.0), (do.wave[10], 30.0)]  # 60 and 70 pixels
    wide = narrow + [(do.wave[200], 37.0)]  # 148 pixels
    lo, hi = D.local_scan_patches(do.wave, wide)
    assert (hi - lo + 1).tolist() == [60, 70, 148]
    out = do.local_scan(None, rows, wide, solver="auto")
    assert do.calls == [("local_scan_batch", 3, 3)] and (out["quad"] == 1.0).all()
    del do.calls[:]
    out = do.local_scan(None, rows, narrow, solver="auto")
    assert do.calls == [("local_scan_banded_batch", 2, 2), ("local_scan_batch", 1, 2)]
    assert out["quad"][:, 0].tolist() == [2.0, 1.0, 2.0] and (out["info"] == 0).all()
    del do.calls[:]
    out = do.local_scan(None, rows, wide, solver="banded")
    assert do.calls == [("local_scan_banded_batch", 2, 3)]
    assert out["info"].tolist() == [0, D.INFO_BANDWIDTH, 0] and np.isnan(out["fisher"][1]).all() and out["lnl"][1] == -np.inf
    del do.calls[:]
    do.local_scan(None, rows, wide)
    do.local_scan(None, rows, wide, solver="dense")
    assert do.calls == [("local_scan_batch", 3, 3)] * 2
    none = FakeOrder(0, [10, 20, 30])
    none.local_scan(None, rows, narrow, solver="auto")
    assert none.calls == [("local_scan_batch", 3, 2)]
    with pytest.raises(ValueError, match="does not take this order"):
        none.local_scan(None, rows, narrow, solver="banded")
    with pytest.raises(ValueError, match="solver must be"):
        none.local_scan(None, rows, narrow, solver="band")
    with pytest.raises(ValueError, match="expected"):
        none.local_scan(None, rows, np.zeros((0, 2)), solver="auto")


class Scan(StandIn):
    limit = 20

    def local_scan_banded_max_patch(self, md):
        self.calls.append("limit")
        return self.limit

    def _result(self, rows, cand, solver):
        B, n = rows.shape[0], len(cand)
        self.calls.append(("local_scan", B, n, solver))
        return dict(quad=np.ones((B, n)), trace=np.zeros((B, n)), fisher=np.ones((B, n)), lnl=np.zeros(B),
                    info=np.full(B, self.info, dtype=np.int32))


class Dense(Scan):
    def local_scan(self, md, rows, cand, max_chunk=None):
        return self._result(rows, cand, None)


class WithSolver(Scan):
    def local_scan(self, md, rows, cand, max_chunk=None, solver="dense"):
        return self._result(rows, cand, solver)


def test_solver_none_is_the_call_as_it_always_was():
    for built_with in ("dense", "auto"):
        model, dev = model_on_a_stand_in(Dense, solver=built_with)
        P = np.tile(model.get_param_vector(), (2, 1))
        state = state_of(model)
        for solver in (None, "dense"):
            model.local_kernel_scan(solver=solver)
            model.local_kernel_scan_batch(P, solver=solver)
            model.propose_local_kernels(solver=solver)
            model.propose_local_kernels(P=P, solver=solver)
        n = dev.n
        assert dev.calls == [("local_scan", 1, 3 * n, None), ("local_scan", 2, 3 * n, None)] * 4
        assert state_of(model) == state


def test_the_band_solvers_are_handed_on_and_banded_holds_the_candidates_to_its_limit():
    model, dev = model_on_a_stand_in(WithSolver)
    wave = np.asarray(model.data.wave)
    P = np.tile(model.get_param_vector(), (3, 1))
    state = state_of(model)
    mus = wave[20:40]
    narrow, wide = (2.0,), (2.0, 30.0)
    lo, hi = D.local_scan_patches(wave, [(wave[30], 2.0), (wave[30], 30.0)])
    assert hi[0] - lo[0] + 1 <= Scan.limit < hi[1] - lo[1] + 1 <= D.LOCAL_SCAN_MAX_PATCH
    for solver in ("banded", "auto"):
        del dev.calls[:]
        assert model.local_kernel_scan(mus=mus, sigmas=narrow, solver=solver)["z"].shape == (1, 20)
        got, info = model.local_kernel_scan_batch(P, mus=mus, sigmas=narrow, return_info=True, solver=solver)
        assert got["score"].shape == (3, 1, 20) and (info == 0).all()
        model.propose_local_kernels(mus=mus, sigmas=narrow, P=P, solver=solver)
        asked = ["limit"] if solver == "banded" else []
        assert dev.calls == asked + [("local_scan", 1, 20, solver)] + (asked + [("local_scan", 3, 20, solver)]) * 2
    # a candidate beyond the banded limit: a ValueError under "banded" before any device call, handed on under "auto"
    del dev.calls[:]
    count = int(hi[1] - lo[1] + 1)
    for call in (lambda **kw: model.local_kernel_scan(mus=mus, sigmas=wide, **kw),
                 lambda **kw: model.local_kernel_scan_batch(P, mus=mus, sigmas=wide, **kw),
                 lambda **kw: model.propose_local_kernels(mus=mus, sigmas=wide, **kw)):
        with pytest.raises(ValueError, match=rf"candidate mu=.*sigma=30\.0 km/s reaches \d+ pixels: the band solver scans patches of at "
                                             rf"most {Scan.limit} pixels \(solver=\"auto\""):
            call(solver="banded")
        assert dev.calls == ["limit"]
        del dev.calls[:]
        call(solver="auto")
        assert [c[3] for c in dev.calls] == ["auto"]
        del dev.calls[:]
    assert count > Scan.limit
    # the device's own limit still holds under every solver
    big, big_dev = model_on_a_stand_in(WithSolver, N=330)
    for solver in (None, "banded", "auto"):
        with pytest.raises(ValueError, match=f"device scans patches of at most {D.LOCAL_SCAN_MAX_PATCH} pixels"):
            big.local_kernel_scan(mus=np.asarray(big.data.wave)[160:170], sigmas=(3000.0,), solver=solver)
    assert all(c == "limit" for c in big_dev.calls)
    for bad in ("band", "Dense", 1):
        with pytest.raises(ValueError, match="solver must be"):
            model.local_kernel_scan(solver=bad)
        with pytest.raises(ValueError, match="solver must be"):
            model.propose_local_kernels(P=P, solver=bad)
    assert state_of(model) == state
    # a failed walker raises as log_likelihood does, whatever the solver
    dev.info = D.INFO_BANDWIDTH
    with pytest.raises(ValueError, match="band"):
        model.local_kernel_scan(mus=mus, sigmas=narrow, solver="banded")
