"""Bit comparison of what the wide Cholesky sequence (panel pairs, k_chol_panel_w) computes, for changes to
starfish_amd/csrc/sf_chol_wide.h that must keep every accumulator's order of operations:
    SF_LIB_PATH=<one build> python tools/potrf_bits.py > a.json
    SF_LIB_PATH=<another>   python tools/potrf_bits.py > b.json
    python tools/potrf_bits.py --compare a.json b.json      -> lists the keys that differ, exit code 1 if any
Prints ONE JSON object {"<case>/<matrix>/<output>": sha256 of the raw bytes} for a fixed, seeded list of cases, every one with
the wide sequence pinned (sf_debug_cholesky_sequence(2)) and three matrices (not a multiple of 8):
  potrf     sf_potrf_batch on well-conditioned random SPD matrices; per matrix the lower triangle of L and info
            n = 640   pair 0 with K = 0 (A slabs 2 and 3 parked, one B slab), pair 1 with K = 256
            n = 1024  the stand-alone call takes multiples of 64 only: the order 1000 of the likelihood case below, padded
            n = 704   64 mod 128: the shifted frame, virtual columns in pair 0
  loglike   sf_loglike_batch (DeviceOrder.loglike, want_resid) with one global and one local kernel, three walkers with
            different tile maps (generated and materialised start tiles): N = 640, N = 1000 (padded order 1024) and N = 704
            (shifted frame); per walker lnl, logdet, sqmah, info and the residual.  The right-hand side z of the factor
            steps is reached through these calls alone (sqmah = |z|^2): the stand-alone factorisation carries none.
The fixture tests/golden/potrf_wide_bits.json is this output from the build BEFORE such a change.  Needs an MI355X."""
import hashlib
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np

BATCH = 3
POTRF_SIZES = (640, 1024, 704)
LOGLIKE_SIZES = (640, 1000, 704)
WIDE = 2


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def spd_batch(n, batch=BATCH):
    """Seeded, well-conditioned: G G^T / n + diag(u), u in [0.5, 2], in rows of n + 16 doubles."""
    rng = np.random.default_rng(n)
    A = np.zeros((batch, n, n + 16))
    for b in range(batch):
        G = rng.standard_normal((n, n))
        A[b, :, :n] = G @ G.T / n + np.diag(rng.uniform(0.5, 2.0, n))
    return A


def potrf_case(out, lib, n):
    import torch
    from starfish_amd import _device as D
    from starfish_amd import _lib

    dev = D.device_of()
    lda = n + 16
    dA = D.to_dev(spd_batch(n), dev)
    info = D.empty((BATCH,), dev, torch.int32)
    ws = D.workspace(lib.sf_potrf_workspace_bytes(n, BATCH), dev)
    _lib.check(lib.sf_potrf_batch(D.ptr(dA), n, lda, n * lda, BATCH, D.ptr(info), D.ptr(ws), ws.numel(), D.stream_ptr(dev)))
    L, info = dA.cpu().numpy(), info.cpu().numpy()
    for b in range(BATCH):
        out[f"potrf-n{n}/{b}/L"] = digest(np.tril(L[b, :, :n]))
        out[f"potrf-n{n}/{b}/info"] = digest(info[b])


def loglike_case(out, N):
    import cov_cases as CC
    from gpu_helpers import device_order, pack_rows

    o = CC.make_grid_order("G1", N, m=8)
    do = device_order(CC.oracle_order_of(o))
    md, rows = pack_rows(do, CC.batch(o, "A", n_local=1))
    res = do.loglike(md, rows, want_resid=True, solver="dense")
    for b in range(BATCH):
        for k in ("lnl", "logdet", "sqmah", "info", "resid"):
            out[f"loglike-N{N}/{b}/{k}"] = digest(res[k][b])
    do.release_workspace()


def main():
    from starfish_amd import _lib

    lib = _lib.require_gpu()
    out = {}
    assert lib.sf_debug_cholesky_sequence(WIDE) == 0
    try:
        for n in POTRF_SIZES:
            potrf_case(out, lib, n)
        for N in LOGLIKE_SIZES:
            loglike_case(out, N)
    finally:
        lib.sf_debug_cholesky_sequence(-1)
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
