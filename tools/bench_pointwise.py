"""Stand-alone timing of sf_pointwise_batch (per-pixel leave-one-out diagnostics) on synthetic orders.
    python tools/bench_pointwise.py [reps] [B] [N ...]
Per N in {3008, 4096}, batch 128, each walker's own residual: ms per call of the whole sf_pointwise_batch, of the new launch
alone (sf_potri_diag_batch: the block inverses and the column norms of L^-1, on synthetic factors of the padded size) and,
beside them from the same run, of sf_apply_batch with SF_APPLY_CINV (everything sf_pointwise_batch does before that launch)
and of sf_potrf_batch on the same synthetic matrices (a factorisation alone)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tests"))
import torch
from gpu_helpers import device_order, oracle_order, pack_rows

from starfish_amd import _device as D
from starfish_amd import _lib, synth

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
B = int(sys.argv[2]) if len(sys.argv) > 2 else 128
sizes = [int(a) for a in sys.argv[3:]] or [3008, 4096]
lib = _lib.require_gpu()


def timed(call, before=None):
    """ms per call; `before` (untimed work, such as restoring an input) runs in front of every call."""
    total = 0.0
    for it in range(reps + 1):  # (the first call is not timed)
        if before:
            before()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        call()
        t1.record()
        torch.cuda.synchronize()
        if it:
            total += t0.elapsed_time(t1)
    return total / reps


for N in sizes:
    o = synth.make_order(N=N, m=4, seed=5)
    do = device_order(oracle_order(o))
    md, rows = pack_rows(do, [synth.vector_to_oracle_params(p) for p in synth.walker_ball(o, B=B)])
    dev, n, npad, lda = do.dev, do.n, do.npad, do.lda
    with torch.cuda.device(dev):
        P = D.to_dev(rows, dev)
        alpha, out = D.empty((B, 1, n), dev), D.empty((B, 1, n), dev)
        cinv_diag, cov_diag = D.empty((B, n), dev), D.empty((B, n), dev)
        info = D.empty((B,), dev, torch.int32)
        ws = do._reserve(do.pointwise_workspace_bytes(md, B, 1))
        whole = timed(lambda: do._call("pointwise_batch", md, B, P, None, 1, n, 0, alpha, cinv_diag, cov_diag, None, info, ws=ws))
        assert int(info.abs().max()) == 0 and bool(torch.isfinite(cinv_diag).all())
        apply = timed(lambda: do._call("apply_batch", md, B, P, 3, None, 1, n, 0, out, None, info, ws=ws))
        assert torch.equal(out, alpha)
        do.release_workspace()
        del ws
        # the new launch alone: factors of the padded size of a diagonally dominant random symmetric matrix, as
        # tools/bench_potrs.py builds it (the kernels' time does not depend on the values)
        g = torch.Generator(device=dev).manual_seed(0)
        base = torch.empty((npad, lda), dtype=torch.float64, device=dev)
        base.normal_(generator=g)
        base[:, :npad] = (base[:, :npad] + base[:, :npad].T) * 0.01
        base[:, :npad] += torch.eye(npad, dtype=torch.float64, device=dev) * 4.0
        A = base.unsqueeze(0).expand(B, npad, lda).contiguous()
        pinfo = torch.empty((B,), dtype=torch.int32, device=dev)
        pws = D.workspace(lib.sf_potrf_workspace_bytes(npad, B), dev)
        potrf = timed(lambda: _lib.check(lib.sf_potrf_batch(D.ptr(A), npad, lda, npad * lda, B, D.ptr(pinfo), D.ptr(pws),
                                                            pws.numel(), D.stream_ptr(dev)), "sf_potrf_batch"),
                      before=lambda: A.copy_(base.unsqueeze(0).expand(B, npad, lda)))
        assert int(pinfo.abs().max()) == 0
        del pws
        d = torch.empty((B, npad), dtype=torch.float64, device=dev)
        iws = D.workspace(lib.sf_potri_diag_workspace_bytes(npad, B), dev)
        alone = timed(lambda: _lib.check(lib.sf_potri_diag_batch(D.ptr(A), npad, lda, npad * lda, B, D.ptr(d), npad, D.ptr(iws),
                                                                 iws.numel(), D.stream_ptr(dev)), "sf_potri_diag_batch"))
        assert bool(torch.isfinite(d).all()) and bool((d[1:] == d[0]).all())
        del iws, A, base, d
    print(f"N={N} B={B}: sf_pointwise_batch {whole:8.3f} ms per call, diag(C^-1) alone {alone:8.3f} ms, "
          f"sf_apply_batch(Cinv) {apply:8.3f} ms, sf_potrf_batch alone {potrf:8.3f} ms", flush=True)
