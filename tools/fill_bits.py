"""Bit comparison of everything the covariance fill feeds, for refactors of starfish_amd/csrc/sf_fill.hip and its layers:
    SF_LIB_PATH=<one build> python tools/fill_bits.py > a.json
    SF_LIB_PATH=<another>   python tools/fill_bits.py > b.json
    python tools/fill_bits.py --compare a.json b.json      -> lists the keys that differ, exit code 1 if any
Prints ONE JSON object {"<case>/<output>": sha256 of the raw bytes the ABI returned} for a fixed, seeded list of small
cases (three walkers each, tests/cov_cases.py) that reach every branch of the fill:
  grids       G1 log-uniform (the likelihood reads K_global from the per-diagonal table), G2 per entry, G4 not monotonic
              (no culling)
  structures  A global + locals, G global only, L locals only, N nothing structured; 32 and 3 local kernels
  sizes       N = 331 (row stride 331: odd, scalar stores; and 336), N = 1050 (padded order 17 x 64: the tile frame shifted
              by 64 under the fused Cholesky sequence), N = 1100 (padded order 9 x 128); both span more than 8 tiles of 128,
              so the bands of 128 + 64 and 256 + 64 pixels leave tiles inside and outside the maps
  rank        m = 8, 5 (padded) and 32 (mpad > 16: the dense fill falls back to the tile fill)
It hashes results only -- nothing inside the workspace (the order of the tile lists depends on atomics).  Needs an MI355X."""
import hashlib
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np

GRIDS = ("G1", "G2", "G4")
SIZES = (331, 1050, 1100)
STRUCTURES = (("A", 32), ("A", 3), ("G", 0), ("L", 32), ("N", 0))
RANK_CASES = (("G1", 331, 5), ("G1", 331, 32), ("G2", 1050, 5), ("G2", 1050, 32))  # with structures A32 and N


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def run_case(out, key, do, o, grid, kind, n_local, lib):
    import cov_cases as CC
    from gpu_helpers import pack_rows

    md, rows = pack_rows(do, CC.batch(o, kind, n_local=n_local))
    n = do.n
    for ld in (n, 336) if n == 331 else (n,):
        for lower in (0, 1):
            for jitter in (0, 1):
                cov, info = do.cov_fill(md, rows, ld=ld, lower_only=bool(lower), add_jitter=bool(jitter))
                out[f"{key}/cov_fill-ld{ld}-lower{lower}-jitter{jitter}"] = digest(np.tril(cov[:, :, :n]) if lower else cov, info)
    fwd = do.forward(md, rows)
    out[f"{key}/forward.cov"] = digest(fwd["cov"], fwd["info"])
    runs = [("auto", dict(solver="dense"), -1), ("fused", dict(solver="dense"), 0)]  # fused: the shifted frame at N = 1050
    if grid != "G4":  # (the banded solver needs a sorted grid)
        runs.append(("banded", dict(solver="banded"), -1))
    for name, kw, seq in runs:
        assert lib.sf_debug_cholesky_sequence(seq) == 0
        res = do.loglike(md, rows, **kw)
        lib.sf_debug_cholesky_sequence(-1)
        out[f"{key}/loglike-{name}"] = digest(*[res[k] for k in ("lnl", "logdet", "sqmah", "info")])
    for nrhs in (1, 17):
        rhs = None if nrhs == 1 else np.random.default_rng(17).standard_normal((nrhs, n))
        res = do.decompose(md, rows, rhs=rhs)
        out[f"{key}/decompose-nrhs{nrhs}.comp"] = digest(res["comp"], res["info"])
        out[f"{key}/decompose-nrhs{nrhs}.alpha"] = digest(res["alpha"])


def main():
    import cov_cases as CC
    from gpu_helpers import device_order
    from starfish_amd import _lib
    from starfish_amd.models import kernels

    lib = _lib.require_gpu()
    out = {}
    orders = [(g, n, 8, STRUCTURES) for g in GRIDS for n in SIZES]
    orders += [(g, n, m, (("A", 32), ("N", 0))) for g, n, m in RANK_CASES]
    for grid, n, m, structures in orders:
        o = CC.make_grid_order(grid, n, m=m)
        do = device_order(CC.oracle_order_of(o))
        for kind, n_local in structures:
            run_case(out, f"{grid}-N{n}-m{m}-{kind}{n_local}", do, o, grid, kind, n_local, lib)
        if n == 331 and m == 8:  # the stand-alone kernels: a band of 40 pixels, a patch in the middle of the order
            w = o["wave"]
            ls = 40 * CC.pixel_metric(w) / 6
            out[f"{grid}-N{n}/sf_global_cov"] = digest(kernels.global_covariance_matrix(w, 3e-3, ls))
            out[f"{grid}-N{n}/sf_local_cov"] = digest(kernels.local_covariance_matrix(w, 2e-3, w[n // 2], 25.0))
        do.release_workspace()
    print(json.dumps(out, sort_keys=True))


def compare(path_a, path_b):
    a, b = (json.loads(open(p).read().strip().splitlines()[-1]) for p in (path_a, path_b))
    bad = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    for k in bad:
        print("DIFFERS:", k)
    print(f"{len(a)} / {len(b)} digests, {len(bad)} differ")
    return 1 if bad or not a else 0


if __name__ == "__main__":
    sys.exit(compare(*sys.argv[2:4]) if sys.argv[1:2] == ["--compare"] else main())
