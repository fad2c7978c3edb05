"""Both forms of the band solver's window sweep at the matrix level, through sf_debug_band_forms_batch: form 0, the single sweep
(k_band_forms with nhalf = 1, what sf_band_logdet_gram_batch runs), and form 1, the two-sided sweep of the likelihood
(sf_launch_band_forms_twisted: two half sweeps, one of them bottom-up on reversed indices, k_band_merge, a third sweep over the
merged separator).  Needs an MI355X.

Shapes, matrix families, the np.longdouble reference and the bounds are those of tests/band_sweep_reference.py: the smallest
orders that reach every window size (nbr 3 .. 10), wave count (8, 12, 16), number of right-hand-side blocks (1 .. 3) and both
parities of the split, at the edges nblk = 6 nbr (where the likelihood starts to take the two-sided form) and nblk = 3 nbr - 1
(the least it fits).  Every call runs on a workspace filled with the bytes 0xff (NaN wherever a double is read before it is
written) and with outputs one element longer than the batch, whose last element must survive."""
import types

import numpy as np
import pytest

from starfish_amd import _device as D
from starfish_amd import _lib

import band_sweep_reference as SW
from test_gpu_fisher import twists

pytestmark = pytest.mark.gpu

SENTINEL, INFO_SENTINEL = -7.25, -77


def packed(bands, ldb, rhs):
    """The layout of a call without padding: bands (batch, n, ldb), rhs (batch, nrhs, n)."""
    batch, n, _ = bands.shape
    nrhs = rhs.shape[1]
    return dict(band=bands.reshape(batch, -1), n=n, ldb=ldb, stride=n * ldb, batch=batch, rhs=rhs.reshape(batch, -1), nrhs=nrhs,
                ldr=n, rhs_stride=nrhs * n)


def padded(bands, w, rhs):
    """The same matrices and right-hand sides with NaN wherever the call has no business: ldb = w + 5 with NaN beyond column
    w and in every entry with d > i, ldr = n + 3 with NaN padding, and a NaN gap behind every matrix and block of rows."""
    batch, n, _ = bands.shape
    nrhs, ldb, ldr = rhs.shape[1], w + 5, n + 3
    stride, rhs_stride = n * ldb + 7, nrhs * ldr + 5
    wide = np.full((batch, n, ldb), np.nan)
    wide[:, :, :w + 1] = bands[:, :, :w + 1]
    wide[:, ~SW.BS.on_band(n, ldb - 1)] = np.nan
    band = np.full((batch, stride), np.nan)
    band[:, :n * ldb] = wide.reshape(batch, -1)
    rows = np.full((batch, nrhs, ldr), np.nan)
    rows[:, :, :n] = rhs
    r = np.full((batch, rhs_stride), np.nan)
    r[:, :nrhs * ldr] = rows.reshape(batch, -1)
    return dict(band=band, n=n, ldb=ldb, stride=stride, batch=batch, rhs=r, nrhs=nrhs, ldr=ldr, rhs_stride=rhs_stride)


def run(lay, w, form, entry="debug"):
    """(logdet, gram, info) of one call; ``entry`` = "stage": sf_band_logdet_gram_batch instead."""
    import torch

    lib = _lib.require_gpu()
    dev = D.device_of()
    batch, nrhs, n = lay["batch"], lay["nrhs"], lay["n"]
    d_band, d_rhs = D.to_dev(lay["band"], dev), D.to_dev(lay["rhs"], dev)
    logdet = torch.full((batch + 1,), SENTINEL, dtype=torch.float64, device=dev)
    gram = torch.full((batch + 1, nrhs, nrhs), SENTINEL, dtype=torch.float64, device=dev)
    info = torch.full((batch + 1,), INFO_SENTINEL, dtype=torch.int32, device=dev)
    head = (D.ptr(d_band), n, w, lay["ldb"], lay["stride"], batch, D.ptr(d_rhs), nrhs, lay["ldr"], lay["rhs_stride"], D.ptr(logdet),
            D.ptr(gram), D.ptr(info))
    if entry == "stage":
        _lib.check(lib.sf_band_logdet_gram_batch(*head, D.stream_ptr(dev)), "sf_band_logdet_gram_batch")
    else:
        need = lib.sf_debug_band_forms_workspace_bytes(n, w, batch, nrhs, form)
        assert (need == 0) == (form == 0)
        ws = torch.full((max(need, 8),), 0xFF, dtype=torch.uint8, device=dev)
        _lib.check(lib.sf_debug_band_forms_batch(*head, form, D.ptr(ws) if form else None, need, D.stream_ptr(dev)),
                   "sf_debug_band_forms_batch")
    logdet, gram, info = logdet.cpu().numpy(), gram.cpu().numpy(), info.cpu().numpy()
    assert logdet[batch] == SENTINEL and (gram[batch] == SENTINEL).all() and info[batch] == INFO_SENTINEL
    # (the inputs are the caller's: not written)
    assert d_band.cpu().numpy().tobytes() == np.ascontiguousarray(lay["band"]).tobytes()
    return logdet[:batch], gram[:batch], info[:batch]


def same_bits(a, b):
    return all(np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes() for x, y in zip(a, b))


def dominant_batch(seed, n, w, nrhs, batch=3):
    rng = np.random.default_rng(seed)
    mats = [SW.dominant(rng, n, w) for _ in range(batch)]
    return np.stack([m[1] for m in mats]), mats[0][2], rng.standard_normal((batch, nrhs, n))


# ------------------------------------------------------------------------------------------ 1. accuracy
@pytest.mark.parametrize("family,n,w,nrhs", SW.CASES)
def test_both_forms_within_the_reference_bounds(family, n, w, nrhs):
    c = SW.case(family, n, w, nrhs)
    lay = packed(c["bands"], c["ldb"], c["rhs"])
    for form in c["forms"]:
        logdet, gram, info = run(lay, w, form)
        assert (info == 0).all(), info
        worst = dict(logdet=0.0, gram=0.0, floor_logdet=0.0, floor_gram=0.0)
        for b in range(SW.BATCH):
            k = SW.checked(c, b)
            ref, bd = k["ref"], k["bounds"][form]
            el = float(abs(SW.LD(logdet[b]) - ref["logdet"]))
            eg = np.abs(gram[b].astype(SW.LD) - ref["gram"]).astype(np.float64)
            for key, err in (("logdet", el), ("gram", eg)):
                worst[key] = max(worst[key], float(np.max(err / bd[key])))
                worst["floor_" + key] = max(worst["floor_" + key], float(np.max(err / bd["floor_" + key])))
            np.testing.assert_array_equal(gram[b], gram[b].T)
        print(f"{family} {n}/{w}/{nrhs} form {form}: err / bound logdet {worst['logdet']:.3g} gram {worst['gram']:.3g}; "
              f"err / first-order floor logdet {worst['floor_logdet']:.3g} gram {worst['floor_gram']:.3g}")
        assert worst["logdet"] <= 1 and worst["gram"] <= 1, (form, worst)


# ------------------------------------------------------------------------------------------ 2. failures
FAIL_SHAPES = ((480, 49, 5), (960, 144, 5))
_CLEAN = {}


def fail_case(n, w, nrhs):
    """The batch of a failure case, its clean results per form and the columns to plant in: made once."""
    if (n, w, nrhs) not in _CLEAN:
        bands, ldb, rhs = dominant_batch(7 * n + w, n, w, nrhs)
        nm, kend0, kend1, fits = SW.twist_shape(n, w)
        assert fits
        lo, hi = kend0 * 16, kend0 * 16 + nm  # the separator's columns
        cols = dict(first=0, top=lo // 2 + 3, separator=lo + nm // 2 + 5, bottom=hi + (n - hi) // 2 + 7, last=n - 1)
        assert 0 < cols["top"] < lo <= cols["separator"] < hi <= cols["bottom"] < n - 1
        _CLEAN[n, w, nrhs] = dict(bands=bands, ldb=ldb, rhs=rhs, cols=cols, clean={f: run(packed(bands, ldb, rhs), w, f) for f in (0, 1)})
    return _CLEAN[n, w, nrhs]


@pytest.mark.parametrize("where", ["first", "top", "separator", "bottom", "last"])
@pytest.mark.parametrize("n,w,nrhs", FAIL_SHAPES)
def test_failure_is_numbered_in_the_callers_columns(n, w, nrhs, where):
    f = fail_case(n, w, nrhs)
    j = f["cols"][where]
    bands = f["bands"].copy()
    bands[1, j, 0] = -1.0  # matrix 1 of 3: its pivot j is negative whatever came before
    for form in (0, 1):
        logdet, gram, info = run(packed(bands, f["ldb"], f["rhs"]), w, form)
        print(f"{n}/{w}/{nrhs} form {form}: planted column {j} ({where}), info {info}")
        assert info[1] == j + 1 and info[0] == 0 and info[2] == 0, (form, where, j, info)
        clean = f["clean"][form]
        for b in (0, 2):  # the neighbours are untouched: the bits of the call without a bad matrix
            assert same_bits((logdet[b], gram[b]), (clean[0][b], clean[1][b])), (form, b)


def test_failure_in_both_halves_reports_one_of_them():
    n, w, nrhs = FAIL_SHAPES[0]
    f = fail_case(n, w, nrhs)
    jt, jb = f["cols"]["top"], f["cols"]["bottom"]
    bands = f["bands"].copy()
    bands[1, jt, 0] = bands[1, jb, 0] = -1.0
    info0 = run(packed(bands, f["ldb"], f["rhs"]), w, 0)[2]
    info1 = run(packed(bands, f["ldb"], f["rhs"]), w, 1)[2]
    print(f"planted columns {jt} and {jb}: single sweep {info0}, two half sweeps {info1}")
    assert info0[1] == jt + 1  # one sweep meets the top one first
    assert info1[1] in (jt + 1, jb + 1)  # the halves run side by side: whichever writes first
    assert info0[0] == info0[2] == info1[0] == info1[2] == 0


# ------------------------------------------------------------------------------------------ 3. poisoned layouts
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("n,w,nrhs", [(384, 33, 17), (960, 144, 16)])
def test_padded_layout_gives_the_packed_bits(n, w, nrhs, form):
    bands, ldb, rhs = dominant_batch(3 * n + w, n, w, nrhs)
    want = run(packed(bands, ldb, rhs), w, form)
    got = run(padded(bands, w, rhs), w, form)
    assert (want[2] == 0).all() and np.isfinite(want[0]).all() and np.isfinite(want[1]).all()
    assert same_bits(got, want)


# ------------------------------------------------------------------------------------------ 4. a matrix's bits are its own
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("n,w,nrhs", [(384, 33, 17), (960, 144, 16)])
def test_a_matrix_has_the_same_bits_alone_in_a_batch_and_again(n, w, nrhs, form):
    bands, ldb, rhs = dominant_batch(5 * n + w, n, w, nrhs, batch=5)
    alone = run(packed(bands[2:3], ldb, rhs[2:3]), w, form)
    again = run(packed(bands[2:3], ldb, rhs[2:3]), w, form)
    among = run(packed(bands, ldb, rhs), w, form)
    assert (among[2] == 0).all()
    assert same_bits(alone, again)
    assert same_bits(alone, [x[2:3] for x in among])
    if form == 0:
        assert same_bits(among, run(packed(bands, ldb, rhs), w, 0, entry="stage"))


# ------------------------------------------------------------------------------------------ 5. the dispatch
@pytest.mark.parametrize("n,w,nrhs,batch", [(288, 17, 9, 3), (288, 17, 9, 130), (128, 17, 5, 3), (300, 17, 9, 3), (300, 17, 9, 130)])
def test_form_minus_one_is_the_likelihoods_rule(n, w, nrhs, batch):
    import torch

    dev = D.device_of()
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    # sf_band_twisted_applicable: whole blocks, and sfb_twist_pays at this device's compute units
    expect = n % 16 == 0 and bool(twists(types.SimpleNamespace(dev=dev, n=n), w, batch))
    if ncu == 256:
        assert expect == ((n, batch) == (288, 3))
    if (n, w) == (128, 17):
        assert not expect  # 8 block columns: fits, but far below 6 nbr
    bands, ldb, rhs = dominant_batch(11 * n + w + batch, n, w, nrhs, batch=3)
    reps = -(-batch // 3)
    bands, rhs = np.tile(bands, (reps, 1, 1))[:batch], np.tile(rhs, (reps, 1, 1))[:batch]
    lay = packed(bands, ldb, rhs)
    auto = run(lay, w, -1)
    single = run(lay, w, 0)
    assert (auto[2] == 0).all()
    if n % 16 == 0:
        twisted = run(lay, w, 1)
        assert not same_bits(single[:2], twisted[:2])  # (or the comparison below says nothing)
        assert same_bits(auto, twisted if expect else single)
    else:
        assert same_bits(auto, single)
