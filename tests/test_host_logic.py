"""CPU-only tests: parameter book-keeping of SpectrumModel (mirrors the reference's
tests/test_models/test_models.py parameter tests), FlatterDict, grids, the TOML round trip, and that
the product refuses to compute without a GPU (no CPU fallback)."""
import os
import re

import numpy as np
import pytest

from starfish_amd import Spectrum, synth
from starfish_amd._flatdict import FlatterDict
from starfish_amd.emulator import Emulator
from starfish_amd.models import SpectrumModel
from starfish_amd.utils import calculate_dv, create_log_lam_grid

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def make_model(**over):
    o = synth.make_order(N=128, m=3, seed=9)
    emu = Emulator(o["grid_points"], o["param_names"], o["emu_wl"], o["weights"], o["eigenspectra"],
                   o["w_hat"], o["flux_mean"], o["flux_std"], o["factors"])
    emu._trained = True
    data = Spectrum(o["wave"], o["flux"], sigmas=o["sigma"])
    c = synth.centre_params(o)
    c.update(over)
    gp = c.pop("grid_params")
    return SpectrumModel(emu, data, grid_params=gp, **c)


def test_label_order_matches_reference_convention():
    m = make_model()
    assert m.labels == synth.LABELS  # kwargs order, cheb moved last, then emulator param names
    np.testing.assert_allclose(m.get_param_vector(), synth.centre_vector(dict(wave=m.data.wave)))


def test_get_set_param_vector_roundtrip_and_length_check():
    m = make_model()
    P0 = m.get_param_vector()
    m.set_param_vector(P0 + 1)
    np.testing.assert_allclose(m.get_param_vector(), P0 + 1)
    with pytest.raises(ValueError):
        m.set_param_vector(P0[:-1])


def test_freeze_thaw_groups():
    m = make_model()
    m.freeze("global_cov")
    assert "global_cov:log_amp" not in m.labels and "global_cov" in m.frozen
    m.freeze("local_cov")
    assert not any(k.startswith("local_cov") for k in m.labels)
    m.freeze("cheb")
    assert not any(k.startswith("cheb") for k in m.labels)
    before = m["global_cov:log_amp"]
    m.set_param_dict({"global_cov": {"log_amp": 100.0}})
    assert m["global_cov:log_amp"] == before  # frozen values are not overwritten
    m.thaw(["global_cov", "local_cov", "cheb"])
    assert m.labels == synth.LABELS
    m.freeze("all")
    assert m.labels == ()
    m.thaw("all")
    assert m.frozen == []
    m.freeze("vz")
    m.set_param_vector(m.get_param_vector())
    assert "vz" not in m.labels and m["vz"] == 10.0


def test_setitem_getitem_delitem():
    m = make_model()
    m["vsini"] = 12.0
    assert m["vsini"] == 12.0
    m["global_cov:log_amp"] = -3.0
    assert m.params["global_cov"]["log_amp"] == -3.0
    m["cheb:4"] = 0.5
    assert m["cheb"] == [0.01, -0.02, 0, 0.5]
    with pytest.raises(KeyError):
        m["cheb:0"] = 1.0
    with pytest.raises(KeyError):
        m["garbage"] = 1.0
    with pytest.raises(KeyError):
        m["global_cov:garbage"] = 1.0
    m["cheb"] = [0.3]
    assert m["cheb"] == [0.3]
    del m["global_cov"]
    assert "global_cov" not in m.params and m._glob_cov is None
    with pytest.raises(KeyError):
        del m["global_cov"]
    m["T"] = 6100.0
    np.testing.assert_allclose(m.grid_params, [6100.0, 4.2, -0.3])


def test_emulator_covariance_form_switch_is_validated():
    """``emulator_cov``: "code" (X^T Sigma_w^-1 X, spectrum_model.py:334-335: default, parity target) or "paper"
    (Phi Sigma_w Phi^T, docs/api/emulator.rst:105); anything else is rejected at construction."""
    from starfish_amd import synth

    o = synth.make_order(N=128, m=4, seed=1)
    assert synth.build_model(o).emulator_cov == "code"
    assert synth.build_model(o, emulator_cov="paper").emulator_cov == "paper"
    with pytest.raises(ValueError, match="emulator_cov"):
        synth.build_model(o, emulator_cov="docs")


def test_multi_order_data_is_rejected():
    o = synth.make_order(N=64, m=2)
    emu = Emulator(o["grid_points"], o["param_names"], o["emu_wl"], o["weights"], o["eigenspectra"],
                   o["w_hat"], o["flux_mean"], o["flux_std"], o["factors"])
    data = Spectrum(np.vstack([o["wave"]] * 2), np.vstack([o["flux"]] * 2))
    with pytest.raises(ValueError):
        SpectrumModel(emu, data, grid_params=[6050, 4.2, -0.3])


def test_toml_roundtrip(tmp_path):
    m = make_model()
    m.freeze("vz")
    path = tmp_path / "model.toml"
    m.save(path, metadata={"note": "unit test"})
    m2 = make_model(vz=99.0)
    m2.load(path)
    assert m2.params == m.params
    assert m2.frozen == m.frozen
    assert m2["local_cov:0:mu"] == m["local_cov:0:mu"]


def test_flatterdict_semantics():
    fd = FlatterDict({"a": 1, "g": {"x": 2, "y": 3}, "l": [{"mu": 1.0}, {"mu": 2.0}]})
    assert fd.keys() == ["a", "g:x", "g:y", "l:0:mu", "l:1:mu"]
    assert "g" in fd and "g:x" in fd and "g:z" not in fd
    assert fd["l:1:mu"] == 2.0
    fd["g:y"] = 30
    assert fd["g"]["y"] == 30
    assert fd.as_dict()["l"] == [{"mu": 1.0}, {"mu": 2.0}]
    child = fd["g"]
    child["x"] = -2
    assert fd["g:x"] == -2
    del fd["g:x"]
    assert fd.keys() == ["a", "g:y", "l:0:mu", "l:1:mu"]
    flat = FlatterDict()
    flat["p:0:q"] = 5
    assert flat.as_dict() == {"p": {"0": {"q": 5}}}
    assert FlatterDict({"a": {"b": 1}}) == FlatterDict({"a": {"b": 1}})


def test_spectrum_containers():
    w = np.linspace(1e4, 4e4, 24).reshape(2, 12)
    s = Spectrum(w, np.ones_like(w), name="x")
    assert s.shape == (2, 12) and len(s) == 2 and s.sigmas.shape == (2, 12)
    r = s.reshape((4, 6))
    assert r.shape == (4, 6)
    s.shape = (1, 24)
    assert s.shape == (1, 24)
    mask = np.zeros(24, bool)
    mask[5:15] = True
    s1 = Spectrum(w.reshape(-1), np.arange(24.0), masks=mask)
    assert s1[0].wave.shape == (10,) and s1[0].flux[0] == 5.0


def test_log_lambda_grid_properties():
    g = create_log_lam_grid(2.0, 5000.0, 5100.0)
    wl = g["wl"]
    assert len(wl) & (len(wl) - 1) == 0
    assert calculate_dv(wl) <= 2.0
    assert abs(wl[0] - 5000.0) < 1e-9 and abs(wl[-1] - 5100.0) < 1e-9
    with pytest.raises(ValueError):
        create_log_lam_grid(2.0, 5100.0, 5000.0)
    with pytest.raises(ValueError):
        create_log_lam_grid(2.0, -1.0, 5000.0)


def test_c_abi_library_loads_and_exports_every_declared_symbol():
    from starfish_amd import _lib

    lib = _lib.load()  # loading needs no GPU
    header = open(os.path.join(ROOT, "include", "starfish_amd.h")).read()
    declared = set(re.findall(r"\b(sf_[a-z0-9_]+)\s*\(", header))
    assert declared, "no declarations parsed"
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/starfish_amd.h but not exported"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    assert lib.sf_version().startswith(b"starfish_amd")


# sf_potrf_workspace_bytes(n, batch) for batch = 1, 16, 64, 128: the factorisation's scratch layout, byte for byte (its
# sizing and the launchers' carving are one function; a change to either moves these numbers)
POTRF_WORKSPACE_BYTES = {
    64: [404499200, 432176896, 520745728, 638837504],
    128: [404638976, 434413312, 529691392, 656728832],
    3008: [410928896, 535052032, 932246272, 1461838592],
    3072: [411068672, 537288448, 941191936, 1479729920],
    4096: [413305088, 573071104, 1084322560, 1765991168],
    16384: [440142080, 1002462976, 2801890048, 5201126144],
    33024: [476483840, 1583931136, 5127762688, 9852871424],
}


def test_potrf_workspace_bytes_are_pinned():
    from starfish_amd import _lib

    lib = _lib.load()  # loading needs no GPU
    for n, want in POTRF_WORKSPACE_BYTES.items():
        got = [lib.sf_potrf_workspace_bytes(n, b) for b in (1, 16, 64, 128)]
        assert got == want, (n, got, want)


def test_product_fails_loudly_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from starfish_amd import _lib, transforms
    from starfish_amd.models.kernels import global_covariance_matrix

    with pytest.raises(_lib.StarfishAMDError):
        global_covariance_matrix(np.linspace(5000, 5001, 8), 1.0, 1.0)
    with pytest.raises(_lib.StarfishAMDError):
        transforms.rotational_broaden(np.linspace(5000, 5001, 8), np.ones(8), 10.0)
    with pytest.raises(_lib.StarfishAMDError):
        make_model().log_likelihood()


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "starfish_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle|sf_oracle\s+import|oracle/", text, re.M), \
                    f"{f} reaches into oracle/"


def test_band_halfwidth_bound_covers_the_true_support():
    """Host-side bound used to route walkers to the banded solver: never smaller than the true support of
    the reference kernels (oracle restatement of models/kernels.py), and tight to a few pixels."""
    from oracle import sf_oracle as O
    from starfish_amd._device import band_halfwidth_bound

    rng = np.random.default_rng(11)
    for n, dv in ((300, 2.0), (257, 3.7)):
      for jitter in (0.0, 0.2):
          wave = 5000.0 * np.exp(np.arange(n) * dv / 2.99792458e5)
          wave[1:-1] += rng.uniform(-jitter, jitter, n - 2) * np.diff(wave).min()  # not exactly log-uniform
          for ls, sig, mu_i in ((3.0, 6.0, n // 3), (9.0, 2.0, 5), (0.7, 11.0, n - 4)):
              row = np.zeros(6 + 3 + 2 + 3)
              row[5] = np.log(ls)
              row[6 + 3 + 2:] = (wave[mu_i] + 0.01, -8.0, np.log(sig))
              K = O.matern32_global(wave, 1.0, ls)
              L = O.gaussian_local(wave, 1.0, wave[mu_i] + 0.01, sig)
              for has_g, n_loc, M in ((1, 0, K), (0, 1, L), (1, 1, K + L)):
                  ii, jj = np.nonzero(M)
                  true_hw = int(np.abs(ii - jj).max())
                  got = int(band_halfwidth_bound(wave, row, 3, has_g, n_loc, 2)[0])
                  # always a bound; tight to a few pixels on a regular grid (it uses the smallest spacing)
                  assert true_hw <= got, (n, ls, sig, has_g, n_loc, true_hw, got)
                  if jitter == 0 and mu_i == n // 3:  # (a patch cut by the array edge is narrower than the bound)
                      assert got <= true_hw + 4, (n, ls, sig, has_g, n_loc, true_hw, got)
    # a grid that is not strictly increasing cannot use the banded solver at all
    assert band_halfwidth_bound(wave[::-1], row, 3, 1, 1, 2)[0] == np.iinfo(np.int32).max


def test_every_status_code_of_the_header_has_a_python_message():
    """include/starfish_amd.h is the contract: each negative per-item status (SF_INFO_*) must be known to the
    Python layer, which turns it into the reference's exceptions / messages."""
    import re

    from starfish_amd import _device as D

    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "starfish_amd.h")).read()
    codes = {name: int(val) for name, val in re.findall(r"#define\s+(SF_INFO_[A-Z_]+)\s+\((-\d+)\)", text)}
    assert len(codes) >= 5, codes
    for name, val in codes.items():
        assert val in D.INFO_MESSAGES, (name, val)
    assert D.INFO_BANDWIDTH == codes["SF_INFO_BANDWIDTH"]


def test_echelle_from_orders_checks_labels_and_synth_helpers():
    """Host-only: EchelleModel.from_orders refuses orders whose thawed labels differ; the multi-order synthetic
    helpers keep the shared / per-order split the cfg 3 goldens were generated with."""
    from starfish_amd import synth
    from starfish_amd.models import EchelleModel

    orders = synth.make_echelle(3, N=64, m=2)
    assert orders[1]["wave"][0] == pytest.approx(5000.0 * 1.02)
    models = [synth.build_model(o, freeze=("local_cov",)) for o in orders]
    em = EchelleModel.from_orders(models)
    assert len(em) == 3 and em.labels == synth.SHARED_LABELS
    P = synth.shared_ball(orders[0], B=4)
    assert P.shape == (4, len(synth.SHARED_LABELS))
    p = synth.shared_to_oracle_params(orders[2], P[1])
    assert p["local_cov"][0][0] == pytest.approx(orders[2]["wave"][64 // 3])  # the order's OWN local kernel
    assert p["grid"] == list(P[1][-3:])
    models[1].thaw("local_cov")
    with pytest.raises(ValueError):
        EchelleModel.from_orders(models)
    with pytest.raises(ValueError):
        EchelleModel.from_orders([])
    # freeze / thaw bookkeeping of a group (table-driven implementation): members are listed once, thaw restores
    m = models[0]
    before = m.labels
    m.thaw("local_cov")
    assert "local_cov:0:mu" in m.labels and "local_cov" not in m.frozen
    m.freeze("local_cov")
    assert m.labels == before and m.frozen.count("local_cov:0:mu") == 1
    with pytest.raises(ValueError):
        m.thaw("global_cov")  # not frozen: list.remove raises, like the reference


def test_bench_builds_through_the_product_and_keeps_the_oracle_in_the_baseline_leg():
    """bench.py must not depend on the test tree, and may touch the oracle only inside the cpu_baseline functions."""
    import ast

    src = open(os.path.join(ROOT, "bench.py")).read()
    assert "gpu_helpers" not in src and '"tests"' not in src
    tree = ast.parse(src)
    allowed = {"_cpu_pool_worker", "cpu_baseline"}
    for fn in [n for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.Module))]:
        name = getattr(fn, "name", "<module>")
        body = fn.body if isinstance(fn, ast.Module) else fn.body
        for node in body if isinstance(fn, ast.Module) else ast.walk(fn):
            if isinstance(node, ast.ImportFrom) and node.module and node.module.split(".")[0] == "oracle":
                assert name in allowed, f"oracle imported in {name}"
            if isinstance(node, ast.Import) and any(a.name.split(".")[0] == "oracle" for a in node.names):
                assert name in allowed, f"oracle imported in {name}"


def test_release_library_has_no_environment_switches():
    """The shipped library must not contain a knob that changes its results or launch sequence from the environment
    (round-2 finding: SF_PANEL_SKIP returned wrong likelihoods by design).  The tuning switches are compiled only
    under -DSF_TUNING (`make TUNING=1` -> libstarfish_amd_tuning.so); the sources reach the environment through
    the SF_TUNE_* macros alone."""
    from starfish_amd import _lib

    blob = open(os.path.join(ROOT, "starfish_amd", "libstarfish_amd.so"), "rb").read()
    for name in (b"SF_PANEL_SKIP", b"SF_CHOL_UNFUSED", b"SF_CHOL_SPLIT", b"SF_NO_LOOKAHEAD", b"SF_MULTI_FIRST",
                 b"SF_BAND_NO_TWIST", b"SF_BAND_TILES_POISON", b"SF_DIAG_SCRATCH"):
        assert name not in blob, name
    assert os.path.basename(_lib.LIB_PATH) == "libstarfish_amd.so"
    csrc = os.path.join(ROOT, "starfish_amd", "csrc")
    for f in os.listdir(csrc):
        if f.endswith((".hip", ".cpp", ".h")):
            for ln in open(os.path.join(csrc, f)):
                if "getenv" in ln:
                    assert f == "sf_common.h" and "#define SF_TUNE_" in ln, (f, ln)


def test_a_library_that_lacks_a_declared_entry_point_does_not_load_silently(monkeypatch):
    """Advisor, round 5: with SF_LIB_PATH set, load() used to skip any missing symbol, so a stale build loaded without
    complaint and failed later inside an error path.  A missing symbol now raises at load time; an OLDER build for a
    same-box A/B has to be asked for (SF_ALLOW_OLD_LIB=1) and every skipped name is reported."""
    from starfish_amd import _lib

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib.SIGNATURES, "sf_entry_point_of_a_newer_header", (None, []))
    monkeypatch.delenv("SF_ALLOW_OLD_LIB", raising=False)
    with pytest.raises(_lib.StarfishAMDError, match="does not export sf_entry_point_of_a_newer_header"):
        _lib.load()
    monkeypatch.setenv("SF_LIB_PATH", _lib.LIB_PATH)
    with pytest.raises(_lib.StarfishAMDError, match="stale or mismatched"):
        _lib.load()  # (the development hook alone does not relax it)
    monkeypatch.setenv("SF_ALLOW_OLD_LIB", "1")
    with pytest.warns(RuntimeWarning, match="lacks sf_entry_point_of_a_newer_header"):
        assert _lib.load() is not None
    monkeypatch.setattr(_lib, "_lib", None)


def test_header_documents_no_environment_switch_and_the_persistent_kernel_status():
    text = open(os.path.join(ROOT, "include", "starfish_amd.h")).read()
    assert "environment switches (tuning aids, read once)" not in text
    assert "reads NO environment variable" in text
    assert "sf_persistent_potrf_status" in text and "25 ms" in text
    blob = open(os.path.join(ROOT, "starfish_amd", "libstarfish_amd.so"), "rb").read()
    for name in (b"SF_DF_STALL_MS", b"SF_DF_MISS_CLAIMS", b"SF_DF_TIMEOUT_S", b"SF_WIDE_HEAD", b"getenv"):
        assert name not in blob, name


def test_multiplan_collect_raises_when_the_internal_status_survives_the_retry(monkeypatch):
    """Advisor, round 5: MultiPlan.collect re-ran an aborted call once and then handed a SECOND -5 back as an ordinary
    per-unit status.  Host logic only (no device): collect_multi is replaced by a fake that keeps returning -5."""
    from starfish_amd import _device as D
    from starfish_amd import _multi

    class FakeLib:
        def __init__(self):
            self.switched = []

        def sf_persistent_potrf_status(self, buf):
            for i, v in enumerate((1, 2, 400, 512, 3_000_000, 77, 1, 1)):
                buf[i] = v
            return 0

        def sf_persistent_potrf(self, v):
            self.switched.append(v)
            return 1

    plan = D.MultiPlan.__new__(D.MultiPlan)
    plan.lib, plan.quad, plan.info, plan.sizes = FakeLib(), None, None, [2]
    calls = []
    plan.enqueue = lambda: calls.append("enqueue")
    bad = [dict(lnl=np.full(2, -np.inf), logdet=np.zeros(2), sqmah=np.zeros(2), log_scale=np.zeros(2),
                info=np.full(2, D.INFO_INTERNAL, dtype=np.int32))]
    monkeypatch.setattr(_multi, "collect_multi", lambda quad, info, sizes: bad)
    with pytest.warns(RuntimeWarning, match="no task of the launch completed for 25 ms; only 400 of its 512 workgroups had started"):
        with pytest.raises(RuntimeError, match="internal error"):
            plan.collect()
    assert calls == ["enqueue"] and plan.lib.switched == [0]
    # ... and a retry that succeeds is returned
    good = [dict(bad[0], info=np.zeros(2, dtype=np.int32), lnl=np.ones(2))]
    seq = iter([bad, good])
    monkeypatch.setattr(_multi, "collect_multi", lambda quad, info, sizes: next(seq))
    with pytest.warns(RuntimeWarning, match="disabled for this whole process"):
        out = plan.collect()
    assert (out[0]["info"] == 0).all()


class _RecoveryLib:
    """What the retry policy touches of the library: the abort record and the process-wide switch."""

    def __init__(self):
        self.switched = []

    def sf_persistent_potrf_status(self, buf):
        for i, v in enumerate((1, 2, 400, 512, 3_000_000, 77, 1, 1)):
            buf[i] = v
        return 0

    def sf_persistent_potrf(self, v):
        self.switched.append(v)
        return 1


def test_retry_internal_runs_once_when_clean_twice_after_an_abort_and_raises_when_it_survives(recwarn):
    from starfish_amd import _device as D

    clean, aborted = np.zeros(3, dtype=np.int32), np.array([0, D.INFO_INTERNAL, D.INFO_INTERNAL], dtype=np.int32)

    def evaluator(script, seen):
        results = iter(script)

        def evaluate(again):
            seen.append(again)
            info = next(results)
            return ("value", len(seen)), info

        return evaluate

    lib, seen = _RecoveryLib(), []
    assert D.retry_internal(lib, "here", evaluator([clean], seen)) == ("value", 1)
    assert seen == [False] and lib.switched == [] and len(recwarn) == 0

    lib, seen = _RecoveryLib(), []
    with pytest.warns(RuntimeWarning, match=r"here: internal status -5 for 2 unit\(s\)") as caught:
        assert D.retry_internal(lib, "here", evaluator([aborted, clean], seen)) == ("value", 2)
    assert seen == [False, True] and lib.switched == [0] and len(caught) == 1

    lib, seen = _RecoveryLib(), []
    with pytest.warns(RuntimeWarning, match="disabled for this whole process"):
        with pytest.raises(RuntimeError, match="internal error"):
            D.retry_internal(lib, "here", evaluator([aborted, aborted], seen))
    assert seen == [False, True] and lib.switched == [0]


def test_structured_tail_keeps_the_banded_values_and_sends_the_rest_to_dense_once_in_index_order(recwarn):
    """finish_structured, the tail the likelihood's and the gradients' band dispatchers share, on stub callbacks: eight walkers,
    0 2 4 7 served by the banded calls, 1 not fitting (still as refused_output made it), 3 flagged -4 by a kernel, 5 and 6 with
    the internal status."""
    from starfish_amd import _device as D

    fits = np.array([True, False, True, True, True, True, True, True])
    codes = np.array([0, D.INFO_BANDWIDTH, 0, D.INFO_BANDWIDTH, 0, D.INFO_INTERNAL, D.INFO_INTERNAL, -2], dtype=np.int32)
    rng = np.random.default_rng(8)

    def banded_results():
        out = D.refused_output(8, dict(grad=(3,), flux=(5,)))
        assert list(out) == ["lnl", "grad", "flux", "info"] and out["info"].dtype == np.int32 and out["grad"].shape == (8, 3)
        assert (out["info"] == D.INFO_BANDWIDTH).all() and np.isneginf(out["lnl"]).all()
        assert np.isnan(out["grad"]).all() and np.isnan(out["flux"]).all()
        served = np.nonzero(fits)[0]
        out["lnl"][served], out["grad"][served], out["flux"][served] = rng.random(7), rng.random((7, 3)), rng.random((7, 5))
        out["info"][:] = codes
        out["lnl"][3], out["grad"][3] = -np.inf, np.nan
        return out

    def dense_stub(seen):
        def dense(rest):
            seen.append(rest.tolist())
            return dict(lnl=100.0 + rest, grad=np.repeat(200.0 + rest, 3).reshape(-1, 3), flux=np.repeat(300.0 + rest, 5).reshape(-1, 5),
                        info=np.zeros(rest.size, dtype=np.int32))

        return dense

    for solver, redone in (("banded", [5, 6]), ("auto", [1, 3, 5, 6])):
        before, seen = banded_results(), []
        want = {key: v.copy() for key, v in before.items()}
        with pytest.warns(RuntimeWarning, match=r"banded solver: internal status -5 for 2 walker\(s\); recomputed densely") as caught:
            out = D.finish_structured(before, fits, solver, dense_stub(seen))
        assert len(caught) == 1 and os.path.samefile(caught[0].filename, __file__)  # attributed to the dispatcher that called
        assert seen == [redone] and out is before
        kept = np.setdiff1d(np.arange(8), redone)
        for key in want:  # bit for bit, the NaN and -inf of the refused walkers included
            assert out[key][kept].tobytes() == want[key][kept].tobytes(), (solver, key)
        assert out["info"][redone].tolist() == [0] * len(redone) and out["lnl"][redone].tolist() == [100.0 + i for i in redone]
        assert (out["grad"][redone] == 200.0 + np.array(redone)[:, None]).all()
        assert (out["flux"][redone] == 300.0 + np.array(redone)[:, None]).all()
        if solver == "banded":
            assert out["info"][[1, 3]].tolist() == [D.INFO_BANDWIDTH] * 2 and np.isneginf(out["lnl"][[1, 3]]).all()
    # nothing to redo: no warning, no dense call
    clean = D.refused_output(3, dict(logdet=()))
    clean["info"][:], clean["lnl"][:] = 0, 1.0
    D.finish_structured(clean, np.ones(3, dtype=bool), "auto", lambda rest: pytest.fail("dense was called"))
    refused = D.refused_output(3, dict(logdet=()))
    D.finish_structured(refused, np.zeros(3, dtype=bool), "banded", lambda rest: pytest.fail("dense was called"))
    assert (refused["info"] == D.INFO_BANDWIDTH).all() and len(recwarn) == 0


def _host_order(monkeypatch, free):
    """A DeviceOrder without a device: ``__new__``, host tensors, and ``free`` bytes reported as free HBM."""
    import contextlib

    import torch
    from starfish_amd import _device as D

    do = D.DeviceOrder.__new__(D.DeviceOrder)
    do.lib, do.dev, do.n, do.ctx, do._ws, do._ws_multi = _RecoveryLib(), torch.device("cpu"), 5, None, None, None
    do._reserve = lambda need: None  # (the workspace is reserved by the chunk loop, once, not by the _call the tests replace)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda dev=None: (free, 2 * free))
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    return do


def test_device_order_loglike_raises_when_the_internal_status_survives_the_retry(monkeypatch):
    """The sibling of the MultiPlan test above: DeviceOrder.loglike handed a second -5 back as a per-walker status."""
    from starfish_amd import _device as D

    do = _host_order(monkeypatch, free=1 << 30)
    do.workspace_bytes = lambda md, B: 1 << 20
    calls = []
    do._call = lambda name, md, B, P, *args, **kw: calls.append((name, B))
    codes = iter([[D.INFO_INTERNAL] * 4, [D.INFO_INTERNAL] * 4, [D.INFO_INTERNAL] * 4, [0] * 4])

    def fetch(quad, info, resid=None):
        assert quad.shape == (4, 4) and info.shape == (4,) and resid is None
        return dict(lnl=np.ones(4), logdet=np.zeros(4), sqmah=np.zeros(4), log_scale=np.zeros(4),
                    info=np.array(next(codes), dtype=np.int32))

    monkeypatch.setattr(D, "fetch_results", fetch)
    with pytest.warns(RuntimeWarning, match=r"sf_loglike_batch: internal status -5 for 4 unit\(s\)") as caught:
        with pytest.raises(RuntimeError, match="internal error"):
            do.loglike(None, np.zeros((4, 9)), max_chunk=3)
    assert calls == [("loglike_batch", 3), ("loglike_batch", 1)] * 2 and do.lib.switched == [0]
    assert [os.path.samefile(w.filename, __file__) for w in caught] == [True]  # attributed to the caller of loglike
    # ... and a retry that succeeds is returned
    with pytest.warns(RuntimeWarning, match="disabled for this whole process"):
        out = do.loglike(None, np.zeros((4, 9)))
    assert (out["info"] == 0).all() and (out["lnl"] == 1).all()


def test_units_that_fit_gives_the_three_chunk_sizes_it_replaced(monkeypatch):
    """The helper against the three expressions it replaced (DeviceOrder.max_batch, MultiPlan and
    Emulator.log_likelihood_batch), written out as they stood: no chunk boundary may move (the Cholesky sequence is
    chosen by batch size)."""
    from starfish_amd import _device as D

    cases = [  # free, held, fixed, per_unit, limit
        (200 << 30, 0, 0, 805_306_368, None),
        (200 << 30, 3 << 30, 1 << 28, 134_217_733, None),
        (1000, 0, 900, 7, None),                  # free * 0.85 < fixed: one unit all the same
        (1 << 30, 1 << 20, 4096, 12_345, 5),      # a limit below what fits
        (1 << 30, 1 << 20, 4096, 12_345, 65535),  # ... far more fit: the emulator's limit holds
        (1 << 30, 0, 4096, 123_456, 65535),       # ... and does not where fewer fit
        (10_000_019, 77, 123, 1, None),
    ]
    got = []
    for free, held, fixed, per_unit, limit in cases:
        do = _host_order(monkeypatch, free)
        got.append(D.units_that_fit(do.dev, fixed, per_unit, held, limit))
        avail = free + held
        multiplan = max(1, (int(avail * 0.85) - fixed) // per_unit)
        if limit:
            multiplan = min(multiplan, int(limit))
        assert got[-1] == multiplan and isinstance(got[-1], int)
        if limit == 65535:  # Emulator.log_likelihood_batch: fixed = 2 * one - two, per_unit = two - one
            one, two = fixed + per_unit, fixed + 2 * per_unit
            assert got[-1] == int(min(max(1, (int(avail * 0.85) - (2 * one - two)) // (two - one)), 65535))
        if fixed == 0 and limit is None:  # DeviceOrder.max_batch
            assert got[-1] == max(1, int(avail * (1.0 - 0.15)) // max(per_unit, 1))
    assert got[2:6] == [1, 5, 65535, 7392]

    # DeviceOrder.max_batch: free HBM plus the workspace it holds, over the workspace of one walker
    import torch

    do = _host_order(monkeypatch, free=100 << 30)
    do.workspace_bytes = lambda md, B: 805_306_368 * B
    assert do.max_batch(None) == max(1, int((100 << 30) * (1.0 - 0.15)) // 805_306_368) == 113
    do._ws = torch.empty(1 << 20, dtype=torch.uint8)
    assert do.max_batch(None) == max(1, int(((100 << 30) + (1 << 20)) * (1.0 - 0.15)) // 805_306_368)
    do.workspace_bytes = lambda md, B: 0
    assert do.max_batch(None) == int(((100 << 30) + (1 << 20)) * (1.0 - 0.15))


def test_grow_workspace_reuses_replaces_and_records_the_stream(monkeypatch):
    from starfish_amd import _device as D
    from starfish_amd import _runtime

    class Buffer:
        def __init__(self, nbytes):
            self.nbytes, self.recorded = nbytes, []

        def numel(self):
            return self.nbytes

        def record_stream(self, stream):
            self.recorded.append(stream)

    made = []

    def factory(nbytes, dev):
        assert slot["ws"] is None  # the old buffer is dropped before the new one is allocated
        made.append(Buffer(nbytes))
        return made[-1]

    monkeypatch.setattr(_runtime, "workspace", factory)
    monkeypatch.setattr(_runtime, "current_stream", lambda dev: ("stream of", dev))
    slot = dict(ws=None)
    first = D.grow_workspace(slot, "ws", 100, "dev0")
    assert first is slot["ws"] is made[0] and first.nbytes == 100 and first.recorded == [("stream of", "dev0")]
    assert D.grow_workspace(slot, "ws", 100, "dev0") is first and D.grow_workspace(slot, "ws", 8, "dev0") is first
    assert len(made) == 1 and len(first.recorded) == 3  # large enough: returned as it is, stream recorded every time
    second = D.grow_workspace(slot, "ws", 101, "dev0")
    assert second is slot["ws"] is made[1] and second is not first and second.nbytes == 101
    assert second.recorded == [("stream of", "dev0")] and len(first.recorded) == 3
