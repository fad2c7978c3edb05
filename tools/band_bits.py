"""Bit comparison of everything the band solver's host layer returns, for refactors of starfish_amd/csrc/sf_banded.cpp and of
the dispatchers in starfish_amd/_device.py and starfish_amd/_multi.py:
    SF_LIB_PATH=<one build> python tools/band_bits.py > a.json
    SF_LIB_PATH=<another>   python tools/band_bits.py > b.json
    python tools/band_bits.py --compare a.json b.json      -> lists the keys that differ, exit code 1 if any
Prints ONE JSON object {"<case>/<output>": sha256 of the raw bytes returned, "<case>/bytes:<query>": integer result of a size
query} for a fixed, seeded list of small cases (three walkers unless said otherwise) taken from the band solver's GPU tests, so
that every branch of the likelihood's head runs once:
  likelihood  (DeviceOrder.loglike, want_resid) "banded" and "auto" at N = 256 (single window sweep), also with max_chunk = 1;
              N = 640, batch 4 (two half sweeps) and 130 (one sweep each); N = 1024 beyond the window (tiles); a narrow, a
              wide and an absurdly wide walker in one call (both groups; "banded" -> -4, "auto" -> dense);
              loglike_banded_device with a half-width below the support (-4 from the kernel)
  gradients   ("banded" and "auto", want_flux) loglike_mean_grad, loglike_grad and loglike_banded_grad with mean and covariance
              columns, for the cases N180, N256, N330-narrow, N180-m17 and N180-Av of the gradient tests, and N256 with one
              walker beyond the window
  stand-alone sf_band_logdet_gram_batch, sf_band_solve_batch, sf_band_selinv_batch at n = 257, half-width 37
It hashes results only -- nothing inside a workspace.  Needs an MI355X."""
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np

GRAD_CASES = ("N180", "N256", "N330-narrow", "N180-m17", "N180-Av", "N256-wide")
AV_LABELS = ("log_scale", "cheb:1", "cheb:2", "T", "logg", "Z", "Av")


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def put(out, key, res):
    for name, v in res.items():
        out[f"{key}/{name}"] = digest(v)


def order(N, m=4):
    from gpu_helpers import device_order, oracle_order
    from starfish_amd import synth

    o = synth.make_order(N=N, m=m, seed=5)
    return o, device_order(oracle_order(o))


def with_log_ls(p, log_ls):
    return dict(p, global_cov=(p["global_cov"][0], float(log_ls)))


def likelihood_cases(out):
    import torch
    from gpu_helpers import pack_rows
    from starfish_amd import _device as D
    from starfish_amd import synth

    def run(key, do, plist, solvers=("banded", "auto"), **kw):
        md, rows = pack_rows(do, plist)
        W = int(np.minimum(do.halfwidth_bound(md, rows), do.banded_max_halfwidth()).max())
        out[f"{key}/bytes:banded"] = int(do.banded_workspace_bytes(md, len(plist), W))
        for solver in solvers:
            put(out, f"{key}-{solver}", do.loglike(md, rows, want_resid=True, solver=solver, **kw))
        do.release_workspace()

    o, do = order(256)
    plist = [synth.vector_to_oracle_params(p) for p in synth.walker_ball(o, B=3, seed=3)]
    run("loglike-N256", do, plist)
    run("loglike-N256-chunk1", do, plist, max_chunk=1)
    o, do = order(640)
    plist = [synth.vector_to_oracle_params(p) for p in synth.walker_ball(o, B=130)]
    plist = [with_log_ls(p, p["global_cov"][1] - np.log(2.0)) for p in plist]
    run("loglike-N640-B4", do, plist[:4], solvers=("banded",))
    run("loglike-N640-B130", do, plist, solvers=("banded",))
    o, do = order(1024)
    plist = [synth.vector_to_oracle_params(p) for p in synth.walker_ball(o, B=6)]
    wide = [with_log_ls(p, np.log(25.0) + 0.01 * (p["vz"] - 10.0)) for p in plist[:3]]
    run("loglike-N1024-tiles", do, wide, solvers=("banded",))
    run("loglike-N1024-mixed", do, [with_log_ls(wide[0], np.log(5.0)), wide[1], with_log_ls(wide[2], np.log(900.0))])
    md, rows = pack_rows(do, plist[:4])
    P, lnl, info = D.to_dev(rows, do.dev), D.empty((4,), do.dev), D.empty((4,), do.dev, torch.int32)
    do.loglike_banded_device(md, P, 16, lnl, info)  # far below the true support
    put(out, "loglike_banded_device-N1024-W16", dict(lnl=lnl.cpu().numpy(), info=info.cpu().numpy()))


def columns(do, md, labels):
    col = {"vsini": 0, "vz": 1, "log_scale": 2, "T": 6, "logg": 7, "Z": 8}
    col.update({f"cheb:{k + 1}": 6 + do.P + k for k in range(md.n_cheb)})
    col["Av"] = 6 + do.P + md.n_cheb + 3 * md.n_local
    return [col[k] for k in labels]


def gradient_cases(out):
    from gpu_helpers import pack_rows
    from starfish_amd import synth

    for name in GRAD_CASES:
        o, do = order(int(name[1:4]), 17 if name.endswith("m17") else 4)
        plist = [synth.vector_to_oracle_params(p) for p in synth.walker_ball(o, B=3, seed=3)]
        labels = tuple(k for k in synth.LABELS if not k.startswith(("global_cov", "local_cov")))
        if name.endswith("Av"):
            for p in plist:
                del p["vz"], p["vsini"]
                p["Av"] = 0.3
            labels = AV_LABELS
        if name.endswith("narrow"):  # the window slides over most of the matrix
            plist = [with_log_ls(p, np.log(2.0)) for p in plist]
        if name.endswith("wide"):  # one walker beyond the window
            plist[1] = with_log_ls(plist[1], np.log(14.0))
        md, rows = pack_rows(do, plist)
        slots = columns(do, md, labels)
        W = int(np.minimum(do.halfwidth_bound(md, rows), do.banded_window_halfwidth()).max())
        out[f"{name}/bytes:banded_mean_grad"] = int(do.loglike_banded_mean_grad_workspace_bytes(md, 3, W, len(slots)))
        for nslots, want_cov in ((len(slots), 0), (0, 1), (len(slots), 1)):
            out[f"{name}/bytes:banded_grad-{nslots}-{want_cov}"] = int(do.loglike_banded_grad_workspace_bytes(md, 3, W, nslots, want_cov))
        for solver in ("banded", "auto"):
            kw = dict(want_flux=True, solver=solver)
            put(out, f"{name}-{solver}/loglike_mean_grad", do.loglike_mean_grad(md, rows, slots, **kw))
            put(out, f"{name}-{solver}/loglike_grad", do.loglike_grad(md, rows, **kw))
            put(out, f"{name}-{solver}/loglike_banded_grad", do.loglike_banded_grad(md, rows, slots, True, **kw))
        do.release_workspace()


def band_batch(rng, n, w, batch=3):
    """Strictly diagonally dominant band matrices in the lower band storage band[i, d] = A[i, i - d] (row stride even)."""
    ldb = w + 1 + (w + 1) % 2
    bands = np.zeros((batch, n, ldb))
    for band in bands:
        for d in range(1, w + 1):
            band[d:, d] = rng.standard_normal(n - d) * 0.3
        full = np.abs(band[:, 1:]).sum(axis=1)
        for d in range(1, w + 1):
            full[: n - d] += np.abs(band[d:, d])
        band[:, 0] = full + 0.5 + rng.random(n)
    return bands, ldb


def standalone_cases(out, lib, n=257, w=37, nrhs=20):
    import torch
    from starfish_amd import _device as D
    from starfish_amd import _lib

    dev = D.device_of()
    rng = np.random.default_rng(100 * n + w)
    bands, ldb = band_batch(rng, n, w)
    d_band, d_rhs = D.to_dev(bands, dev), D.to_dev(rng.standard_normal((3, nrhs, n)), dev)
    logdet, gram, info = D.empty((3,), dev), D.empty((3, nrhs, nrhs), dev), D.empty((3,), dev, torch.int32)
    host = lambda **kw: {k: v.cpu().numpy() for k, v in kw.items()}  # noqa: E731
    s = D.stream_ptr(dev)
    _lib.check(lib.sf_band_logdet_gram_batch(D.ptr(d_band), n, w, ldb, n * ldb, 3, D.ptr(d_rhs), nrhs, n, nrhs * n, D.ptr(logdet),
                                             D.ptr(gram), D.ptr(info), s), "sf_band_logdet_gram_batch")
    put(out, "sf_band_logdet_gram_batch", host(logdet=logdet, gram=gram, info=info))
    need = out["sf_band_solve_batch/bytes"] = int(lib.sf_band_solve_workspace_bytes(n, w, 3, nrhs))
    ws, x = D.workspace(need, dev), D.empty((3, nrhs, n), dev)
    for name, g in (("gram", gram), ("nogram", None)):  # (no Gram matrix asked for: the workspace's)
        _lib.check(lib.sf_band_solve_batch(D.ptr(d_band), n, w, ldb, n * ldb, 3, D.ptr(d_rhs), nrhs, n, nrhs * n, D.ptr(x), n, nrhs * n,
                                           D.ptr(logdet), D.ptr(g), D.ptr(info), D.ptr(ws), need, s), "sf_band_solve_batch")
        put(out, f"sf_band_solve_batch-{name}", host(x=x, logdet=logdet, gram=gram, info=info))
    need = out["sf_band_selinv_batch/bytes"] = int(lib.sf_band_selinv_workspace_bytes(n, w, 3))
    ws, ldo = D.workspace(need, dev), w + 2
    sel = D.to_dev(np.full((3, n + 1, ldo), 7.0), dev)  # (a row and a column the call leaves alone)
    _lib.check(lib.sf_band_selinv_batch(D.ptr(d_band), n, w, ldb, n * ldb, 3, D.ptr(sel), ldo, (n + 1) * ldo, D.ptr(logdet), D.ptr(info),
                                        D.ptr(ws), need, s), "sf_band_selinv_batch")
    put(out, "sf_band_selinv_batch", host(out=sel, logdet=logdet, info=info))


def main():
    from starfish_amd import _lib

    lib = _lib.require_gpu()
    out = {}
    likelihood_cases(out)
    gradient_cases(out)
    standalone_cases(out, lib)
    print(json.dumps(out, sort_keys=True))


def compare(path_a, path_b):
    a, b = (json.loads(open(p).read().strip().splitlines()[-1]) for p in (path_a, path_b))
    bad = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    for k in bad:
        print("DIFFERS:", k)
    print(f"{len(a)} / {len(b)} entries, {len(bad)} differ")
    return 1 if bad or not a else 0


if __name__ == "__main__":
    sys.exit(compare(*sys.argv[2:4]) if sys.argv[1:2] == ["--compare"] else main())
