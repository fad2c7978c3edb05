"""Stand-alone timing of sf_pointwise_batch (per-pixel leave-one-out diagnostics) on synthetic orders.
    python tools/bench_pointwise.py [reps] [B] [N ...]
Per N in {3008, 4096}, batch 128, each walker's own residual: ms per call of the whole sf_pointwise_batch, of the new launch
alone (sf_potri_diag_batch: the block inverses and the column norms of L^-1, on synthetic factors of the padded size) and,
beside them from the same run, of sf_apply_batch with SF_APPLY_CINV (everything sf_pointwise_batch does before that launch)
and of sf_potrf_batch on the same synthetic matrices (a factorisation alone)."""
import torch
from _bench_common import arguments, dominant_matrices, order_and_walkers, potrf, timed
from gpu_helpers import pack_rows

from starfish_amd import _device as D
from starfish_amd import _lib

reps, B, sizes = arguments(3)
lib = _lib.require_gpu()
for N in sizes:
    o, do, walkers = order_and_walkers(N, B)
    md, rows = pack_rows(do, walkers)
    dev, n, npad, lda = do.dev, do.n, do.npad, do.lda
    with torch.cuda.device(dev):
        P = D.to_dev(rows, dev)
        alpha, out = D.empty((B, 1, n), dev), D.empty((B, 1, n), dev)
        cinv_diag, cov_diag = D.empty((B, n), dev), D.empty((B, n), dev)
        info = D.empty((B,), dev, torch.int32)
        ws = do._reserve(do.pointwise_workspace_bytes(md, B, 1))
        whole = timed(lambda: do._call("pointwise_batch", md, B, P, None, 1, n, 0, alpha, cinv_diag, cov_diag, None, info, ws=ws),
                      reps)
        assert int(info.abs().max()) == 0 and bool(torch.isfinite(cinv_diag).all())
        apply = timed(lambda: do._call("apply_batch", md, B, P, 3, None, 1, n, 0, out, None, info, ws=ws), reps)
        assert torch.equal(out, alpha)
        do.release_workspace()
        del ws
        # the new launch alone: synthetic factors of the padded size
        base, A = dominant_matrices(npad, lda, B, dev, torch.Generator(device=dev).manual_seed(0))
        pinfo = torch.empty((B,), dtype=torch.int32, device=dev)
        pws = D.workspace(lib.sf_potrf_workspace_bytes(npad, B), dev)
        factor = timed(lambda: potrf(lib, A, npad, lda, B, pinfo, pws, dev), reps,
                       before=lambda: A.copy_(base.unsqueeze(0).expand(B, npad, lda)))
        assert int(pinfo.abs().max()) == 0
        del pws
        d = torch.empty((B, npad), dtype=torch.float64, device=dev)
        iws = D.workspace(lib.sf_potri_diag_workspace_bytes(npad, B), dev)
        alone = timed(lambda: _lib.check(lib.sf_potri_diag_batch(D.ptr(A), npad, lda, npad * lda, B, D.ptr(d), npad, D.ptr(iws),
                                                                 iws.numel(), D.stream_ptr(dev)), "sf_potri_diag_batch"), reps)
        assert bool(torch.isfinite(d).all()) and bool((d[1:] == d[0]).all())
        del iws, A, base, d
    print(f"N={N} B={B}: sf_pointwise_batch {whole:8.3f} ms per call, diag(C^-1) alone {alone:8.3f} ms, "
          f"sf_apply_batch(Cinv) {apply:8.3f} ms, sf_potrf_batch alone {factor:8.3f} ms", flush=True)
