"""Host numerics of the C-ABI layer (starfish_amd/csrc/sf_hostmath.cpp) against the CPU oracle, without a GPU.

sf_hostmath.cpp is plain C++: it is compiled here with the host compiler, under AddressSanitizer and
UndefinedBehaviorSanitizer, together with tests/hostmath_driver.cpp (a stand-alone program), which is run as a child
process and prints hex floats.  Nothing is loaded into Python.

Every bound below is 8 x the maximum error measured on the authoring host (g++ 13, glibc), the margin being for another
libm or host compiler; the measured figure stands in each test's docstring.  Exact comparisons have no tolerance."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy.linalg import cho_factor, cho_solve

from oracle import sf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "starfish_amd", "csrc")
SF_EINVAL = -1
SF_KB, SF_IW = 5, 64
# 8 x the measured maximum of each comparison (figures in the tests' docstrings)
LU_BOUND = 8 * 1.110e-16
INV_BOUND = 8 * 1.023e-15
EMU_ALPHA_BOUND = 8 * 6.242e-16
EMU_LINV_BOUND = 8 * 3.184e-16
EXT_BOUND = 8 * 6.811e-15
TW_BOUND = 0.0


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """(path of the driver, sanitized?).  Without the sanitizer runtimes on this host the build falls back to a plain
    one; test_the_driver_runs_under_the_sanitizers then says so."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    out = str(tmp_path_factory.mktemp("hostmath") / "hostmath_driver")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "hostmath_driver.cpp"),
           os.path.join(CSRC, "sf_hostmath.cpp"), os.path.join(CSRC, "sf_error.cpp"), "-o", out]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(cmd + san, capture_output=True, text=True)
    if r.returncode == 0 and subprocess.run([out, "tw"], input="8\n", capture_output=True, text=True).returncode == 0:
        return out, True
    subprocess.run(cmd, check=True)
    return out, False


def run(driver, command, *numbers):
    """One child process; returns (rc, error text, {name: array})."""
    text = "\n".join(float(v).hex() for v in np.concatenate([np.atleast_1d(np.asarray(n, dtype=np.float64)).ravel()
                                                             for n in numbers]))
    r = subprocess.run([driver[0], command], input=text + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    rc = int(lines[0].split()[1])
    err = lines[1][4:]
    vals = {ln.split()[0]: np.array([float.fromhex(t) for t in ln.split()[1:]]) for ln in lines[2:]}
    return rc, err, vals


def test_the_driver_runs_under_the_sanitizers(driver):
    if not driver[1]:
        pytest.skip("no AddressSanitizer / UndefinedBehaviorSanitizer runtime for the host compiler here: "
                    "the host numerics were checked in a plain build")


def nonuniform_grid(n):
    return 5000.0 + np.cumsum(np.random.default_rng(100 + n).uniform(0.5, 1.5, n))


def loguniform_grid(nf):
    return 5000.0 * np.exp(np.arange(nf) * (2.0 / 2.99792458e5))


def dense_collocation(x):
    ab, offs, t = O.quintic_collocation_band(x)
    A = np.zeros((len(x), len(x)))
    for i in range(len(x)):
        A[i, offs[i]:offs[i] + 6] = ab[i]
    return A, t


@pytest.mark.parametrize("n", [6, 7, 16, 64])
def test_knots_and_collocation_lu(driver, n):
    """Knots equal quintic_knots(x) exactly.  L U rebuilt from Lf, Uf, rdiag against the dense collocation matrix of the
    oracle (entries in [0, 1]): measured max |L U - A| = 1.110e-16 (n = 16, 64; 5.551e-17 at n = 6, 7); bound 8 x that = 8.9e-16."""
    x = nonuniform_grid(n)
    rc, err, v = run(driver, "lu", n, x)
    assert rc == 0, err
    A, t = dense_collocation(x)
    assert np.array_equal(v["t"], O.quintic_knots(x)) and np.array_equal(v["t"], t)
    Lf, Uf = v["Lf"].reshape(n, SF_KB), v["Uf"].reshape(n, SF_KB)
    L, U = np.eye(n), np.diag(1.0 / v["rdiag"])
    for j in range(n):
        for k in range(1, SF_KB + 1):
            if j - k >= 0:
                L[j, j - k] = Lf[j, k - 1]
            if j + k < n:
                U[j, j + k] = Uf[j, k - 1]
    e = np.abs(L @ U - A).max()
    print(f"n={n}: max |LU - A| = {e:.3e}")
    assert e <= LU_BOUND


def test_collocation_lu_refuses_bad_grids(driver):
    x = nonuniform_grid(5)
    rc, err, _ = run(driver, "lu", 5, x)
    assert rc == SF_EINVAL and err == "resample needs at least 6 points, got 5"
    x = nonuniform_grid(8)
    x[4] = x[3]
    rc, err, _ = run(driver, "lu", 8, x)
    assert rc == SF_EINVAL and err == "resample: the source grid must be strictly increasing"


@pytest.mark.parametrize("nf", [64, 256])
def test_truncated_inverse_and_its_block_repack(driver, nf):
    """y = A c on a log-uniform grid (nf = 64: every window clipped on both sides; 256: interior windows); the band and
    its 16 x 16 repack applied to y recover c: measured max |c' - c| / max |c| = 1.023e-15 (nf = 256; 5.265e-16 at 64); bound 8 x that = 8.2e-15.  The repack
    holds the same numbers plus exact zeros and both products sum over ascending columns: equal bits."""
    x = loguniform_grid(nf)
    A, _ = dense_collocation(x)
    c = np.random.default_rng(nf).standard_normal(nf)
    rc, err, v = run(driver, "inv", nf, x, A @ c)
    assert rc == 0, err
    assert v["sizes"].tolist() == [(2 * SF_IW + 1) * nf, (nf // 16) * (2 * (SF_IW // 16) + 1) * 256]
    assert np.array_equal(v["c_band"], v["c_blocks"])
    e = np.abs(v["c_band"] - c).max() / np.abs(c).max()
    print(f"nf={nf}: max |c' - c| / max |c| = {e:.3e}")
    assert e <= INV_BOUND


@pytest.mark.parametrize("m,M", [(2, 3), (4, 6)])
def test_emulator_constants(driver, m, M):
    """alpha against cho_solve and Linv against the inverse of numpy's Cholesky factor, N = m M = 6 and 24 (v11 = G G^T + N I,
    condition number below 10): measured max errors, normalised by the largest entry, 6.242e-16 (alpha) and 3.184e-16 (Linv)
    at N = 24 (2.018e-16, 1.567e-16 at N = 6); bounds 8 x that = 5.0e-15 and 2.6e-15."""
    N = m * M
    rng = np.random.default_rng(N)
    G = rng.standard_normal((N, N))
    v11 = G @ G.T + N * np.eye(N)
    w_hat = rng.standard_normal(N)
    rc, err, v = run(driver, "emu", N, v11, w_hat)
    assert rc == 0, err
    alpha = cho_solve(cho_factor(v11), w_hat)
    Linv = np.linalg.inv(np.linalg.cholesky(v11))
    ea = np.abs(v["alpha"] - alpha).max() / np.abs(alpha).max()
    el = np.abs(v["Linv"].reshape(N, N) - Linv).max() / np.abs(Linv).max()
    print(f"N={N}: alpha {ea:.3e}, Linv {el:.3e}")
    assert ea <= EMU_ALPHA_BOUND and el <= EMU_LINV_BOUND


def test_emulator_constants_refuse_an_indefinite_matrix(driver):
    v11 = np.eye(6)
    v11[3, 3] = -1.0
    rc, err, _ = run(driver, "emu", 6, v11, np.ones(6))
    assert rc == SF_EINVAL and err == "emulator v11 is not positive definite (row 3)"


def oracle_spline_law(law, r_v, monkeypatch):
    """Anchors of the oracle's law and its natural CubicSpline (both live inside the oracle's function)."""
    import scipy.interpolate

    seen = {}
    real = scipy.interpolate.CubicSpline

    def recorder(xk, yk, **kw):
        seen["xk"], seen["yk"], seen["spline"] = np.array(xk), np.array(yk), real(xk, yk, **kw)
        assert kw == {"bc_type": "natural"}
        return seen["spline"]

    monkeypatch.setattr(scipy.interpolate, "CubicSpline", recorder)
    wave = np.array([5000.0])
    O.fitzpatrick99_a_lambda(wave, 1.0, r_v) if law == 3 else O.fm07_a_lambda(wave, 1.0)
    monkeypatch.undo()
    return seen["xk"], seen["yk"], seen["spline"](seen["xk"], 2)


@pytest.mark.parametrize("law,r_v", [(3, 3.1), (3, 2.5), (4, 3.1)])
def test_extinction_spline_table(driver, law, r_v, monkeypatch):
    """Anchors equal the oracle's exactly; y'' against the second derivatives of scipy's natural CubicSpline through them:
    measured max |y'' - y''_scipy| / max |y''| = 6.811e-15 (law 4; 5.534e-15 and 4.911e-15 for law 3 at Rv 3.1, 2.5);
    bound 8 x that = 5.5e-14."""
    xk, yk, y2 = oracle_spline_law(law, r_v, monkeypatch)
    rc, err, v = run(driver, "ext", law, r_v)
    assert rc == 0, err
    tab = v["tab"]
    nk = int(tab[0])
    assert nk == len(xk) and len(tab) == 9 + 3 * nk
    assert np.array_equal(tab[9:9 + nk], xk)
    assert np.array_equal(tab[9 + nk:9 + 2 * nk], yk), (tab[9 + nk:9 + 2 * nk] - yk)
    e = np.abs(tab[9 + 2 * nk:] - y2).max() / np.abs(y2).max()
    print(f"law {law} Rv {r_v}: y'' {e:.3e}")
    assert e <= EXT_BOUND


def test_fm07_is_refused_off_its_rv(driver):
    rc, err, _ = run(driver, "ext", 4, 3.0)
    assert rc == SF_EINVAL and err == "fm07 is defined for Rv = 3.1 only"


@pytest.mark.parametrize("nf", [8, 4096])
def test_twiddles(driver, nf):
    """exp(-2 pi i k / nf) against numpy in longdouble, rounded to double: measured max difference 0 at both sizes (numpy's
    longdouble cos / sin are the same libm's cosl / sinl): bound 8 x that = 0, an exact comparison."""
    rc, _, v = run(driver, "tw", nf)
    k = np.arange(nf // 2, dtype=np.longdouble)
    ang = np.longdouble(-2) * np.longdouble("3.14159265358979323846264338327950288") * k / np.longdouble(nf)
    want = np.stack([np.cos(ang), np.sin(ang)], axis=1).astype(np.float64).ravel()
    e = np.abs(v["tw"] - want).max()
    print(f"nf={nf}: max |tw - numpy| = {e:.3e}")
    assert len(v["tw"]) == nf and e <= TW_BOUND


# ---- the band solver's shape (starfish_amd/csrc/sf_band_shape.h): what the kernel, its launchers and the workspace layout
# share, for every half-width 0 .. 160 and every number of right-hand sides 1 .. 49.  The sizes below are written out here
# a second time on purpose (the formulas the launchers used before the header existed): the header has to reproduce them.
BAND_W, BAND_NRHS, BAND_NCU = 160, 49, 256
NEITHER, WINDOW, TILES = 0, 1, 2
BB, BS, PF, PT = 16, 16 * 17, 4, 8


@pytest.fixture(scope="module")
def band(driver):
    rc, err, v = run(driver, "band", BAND_W, BAND_NRHS, BAND_NCU)
    assert rc == 0, err
    assert v["consts"].tolist() == [BB, BS, BB + 1, PF, PT, 160 * 1024, 768]
    grid = (BAND_W + 1, BAND_NRHS)
    return {"maxhw": v["maxhw"].astype(int), "shape": v["shape"].astype(int).reshape(*grid, 5),
            "lds": v["lds"].astype(int).reshape(*grid, 11), "workers": v["workers"].astype(int).reshape(*grid, 16, 2),
            "twist": v["twist"].astype(int).reshape(-1, 6), "carve": v["carve"].astype(np.int64).reshape(-1, 13),
            "pays": v["pays"].astype(int)}


def lds_bytes_before(nbr, nrb):
    """The dynamic LDS size the launcher computed before the shape had a header of its own."""
    nr = nrb * BB
    return 8 * (nbr * (nbr + 1) // 2 * BS + nrb * nbr * BS + 2 * BS + nr * (nr + 1) + 4 * BB + 16 * PT // 2)


def test_band_limits_and_admission(band):
    """Largest half-width of the window: 144, 128, 112 for up to 16, 32, 48 right-hand sides, none beyond; a half-width is
    the window's up to that limit, the tiles' up to 768, nobody's with more than 48 right-hand sides."""
    want = [144 if n <= 16 else 128 if n <= 32 else 112 if n <= 48 else -1 for n in range(1, BAND_NRHS + 1)]
    assert band["maxhw"].tolist() == want
    for w in range(BAND_W + 1):
        for n in range(1, BAND_NRHS + 1):
            admit, nbr, nrb, nwaves, groups = band["shape"][w, n - 1]
            assert nbr == max(3, (w + 31) // 16) and nrb == (n + 15) // 16
            assert nwaves == (8 if nbr <= 4 else 12 if nbr <= 8 else 16) and groups == (nwaves - 4) // 4
            assert admit == (NEITHER if n > 48 else WINDOW if w <= want[n - 1] else TILES), (w, n)
            assert (admit == WINDOW) == (n <= 48 and lds_bytes_before(nbr, nrb) <= 160 * 1024)


def test_band_lds_layout(band):
    """The regions lie in order without overlap and end within the byte count, which is the launcher's earlier formula
    (at most 160 KiB where the window is admitted; 64 bytes of it are a reserve nothing uses)."""
    for w in range(BAND_W + 1):
        for n in range(1, BAND_NRHS + 1):
            admit, nbr, nrb = band["shape"][w, n - 1][:3]
            off, nbytes = band["lds"][w, n - 1][:10], band["lds"][w, n - 1][10]
            nr = nrb * BB
            sizes = [8 * nbr * (nbr + 1) // 2 * BS, 8 * nrb * nbr * BS, 8 * 2 * BS, 8 * nr * (nr + 1), 8 * 2 * BB, 8 * BB,
                     4 * 16, 4 * 16 * PT, 64]  # Wb, RH, Fb2, G, pv, red, sync, ptab, reserve
            assert off[0] == 0 and (off[1:] == off[:-1] + sizes).all(), (w, n)  # each region starts where the last ends
            assert off[9] == nbytes == lds_bytes_before(nbr, nrb)
            assert off[6] % 4 == 0 and off[7] % 4 == 0 and (off[:6] % 8 == 0).all()
            if admit == WINDOW:
                assert nbytes <= 160 * 1024
    at = {(nbr, nrb): None for nbr, nrb in [(3, 1), (10, 1), (9, 2), (8, 3)]}
    for w in range(BAND_W + 1):
        for n in range(1, BAND_NRHS + 1):
            key = tuple(band["shape"][w, n - 1][1:3])
            if key in at:
                at[key] = band["lds"][w, n - 1][10]
    assert at == {(3, 1): 27136, (10, 1): 148992, (9, 2): 150912, (8, 3): 154752}


def test_band_kernel_conditions(band):
    """What k_band_forms relies on for every shape the window admits (its run-time flags guard the same): the loader groups'
    registers cover a block row, no worker is dealt more pairs than its table row holds, two row blocks per worker cover
    the column below wave 0's block, and the workgroup has a thread per element of a right-hand-side column block row."""
    checked = 0
    for w in range(BAND_W + 1):
        for n in range(1, BAND_NRHS + 1):
            admit, nbr, nrb, nwaves, groups = band["shape"][w, n - 1]
            if admit != WINDOW:
                continue
            checked += 1
            RB, nworkers = nbr - 1 + nrb, nwaves - 1
            assert groups * PF >= nbr
            assert 64 * nwaves >= 16 * RB
            pos, pairs = band["workers"][w, n - 1][:, 0], band["workers"][w, n - 1][:, 1]
            assert pos[0] == -1 and (pos[nwaves:] == -1).all()
            assert sorted(pos[1:nwaves]) == list(range(nworkers))  # every position once
            assert pairs[1:nwaves].max() <= PT - 1
            assert pairs[1:nwaves].sum() == RB * (RB + 1) // 2 - 1  # every pair but wave 0's is dealt once
            for p in pos[1:nwaves]:  # the round robin the kernel walks, counted here again
                assert pairs[list(pos).index(p)] == len(range(1 + p, RB * (RB + 1) // 2, nworkers))
            solved = {1 + p + k * nworkers for p in pos[1:nwaves] for k in (0, 1)}
            assert set(range(1, RB)) <= solved
    assert checked == 145 * 16 + 129 * 16 + 113 * 16


def test_band_twisted_shape(band):
    """Two half sweeps and the separator make up the matrix; the workspace's regions are disjoint and add up to the count
    the size query has always given; at 256 compute units batches 1 .. 128 take two half sweeps, 129 .. 256 one, 300 two
    and 1600 one (the cases the rule's comment quotes)."""
    tw = band["twist"]
    assert set(tw[:, 0]) == set(range(3, 12))
    for nbr in range(3, 12):
        rows = tw[tw[:, 0] == nbr]
        assert rows[:, 1].tolist() == list(range(6 * nbr, 301))
    nbr, nblk, nm, k0, k1, fits = tw.T
    assert (nm == 16 * (nbr - 1)).all() and (k0 + k1 + nbr - 1 == nblk).all() and (abs(k0 - k1) <= 1).all()
    assert (np.minimum(k0, k1) >= nbr).all() and fits.all()  # each half sweeps at least a window's length
    carve = band["carve"]
    assert len(carve) == 2 * (145 * 16 + 129 * 16 + 113 * 16)
    for w, n, b, *rest in carve.tolist():
        off, total, counted = rest[:8], rest[8], rest[9]
        nm_, nr = 16 * (max(3, (w + 31) // 16) - 1), 16 * ((n + 15) // 16)
        sizes = [2 * b * nm_ * nm_, 2 * b * nr * nm_, 2 * b * n * n, 2 * b, b * nm_ * nm_, b * nr * nm_, b * n * n, b]
        assert off[0] == 0 and all(off[i] + sizes[i] <= off[i + 1] for i in range(7)) and off[7] + sizes[7] <= total
        assert total == counted == 3 * b * (nm_ * nm_ + nr * nm_ + n * n + 1) + 64
    pays = band["pays"]
    assert pays[:128].all() and not pays[128:256].any() and pays[300 - 1] == 1 and pays[1600 - 1] == 0
    assert pays[1600] == 0  # fewer than 6 nbr block columns: never
