"""Stand-alone timing of sf_decompose_batch (the residual split by covariance component) on synthetic orders.
    python tools/bench_decompose.py [reps] [B] [N ...]
Per N in {3008, 4096}, batch 128, nrhs in {1, 16}: ms per call of the whole sf_decompose_batch, of its last step alone (the
kernels of sf_cov_matvec.h, through sf_debug_decompose_matvec on the workspace the call left) and, beside them, of
sf_apply_batch with SF_APPLY_CINV (everything sf_decompose_batch does before that step) and of sf_potrs_batch with
SF_APPLY_CINV on synthetic factors of the same size (the C^-1 alone, the number tools/bench_potrs.py reports)."""
import ctypes as C

import torch
from _bench_common import arguments, dominant_matrices, factorised, order_and_walkers, timed
from gpu_helpers import pack_rows

from starfish_amd import _device as D
from starfish_amd import _lib

reps, B, sizes = arguments(5)
lib = _lib.require_gpu()
for N in sizes:
    o, do, walkers = order_and_walkers(N, B)
    md, rows = pack_rows(do, walkers)
    dev, n, npad, lda = do.dev, do.n, do.npad, do.lda
    with torch.cuda.device(dev):
        P = D.to_dev(rows, dev)
        g = torch.Generator(device=dev).manual_seed(0)
        # C^-1 alone: sf_potrs_batch on synthetic factors of the padded size
        base, A = dominant_matrices(npad, lda, B, dev, g)
        factorised(lib, A, npad, lda, B, dev)
        del base
        for nrhs in (1, 16):
            rhs = torch.empty((B, nrhs, n), dtype=torch.float64, device=dev)
            rhs.normal_(generator=g)
            comp = D.empty((B, 3 + md.n_local, nrhs, n), dev)
            alpha, out = D.empty((B, nrhs, n), dev), D.empty((B, nrhs, n), dev)
            info = D.empty((B,), dev, torch.int32)
            ws = do._reserve(do.decompose_workspace_bytes(md, B, nrhs))
            whole = timed(lambda: do._call("decompose_batch", md, B, P, rhs, nrhs, n, nrhs * n, comp, alpha, None, info, ws=ws), reps,
                          back_to_back=True)
            assert int(info.abs().max()) == 0
            kept = comp.clone()
            matvec = timed(lambda: _lib.check(lib.sf_debug_decompose_matvec(
                do.ctx, C.byref(md), B, D.ptr(P), nrhs, D.ptr(comp), D.ptr(ws), ws.numel(), D.stream_ptr(dev)),
                "sf_debug_decompose_matvec"), reps, back_to_back=True)
            assert torch.equal(comp, kept)  # the same bits as inside the whole call
            apply = timed(lambda: do._call("apply_batch", md, B, P, 3, rhs, nrhs, n, nrhs * n, out, None, info, ws=ws), reps,
                          back_to_back=True)
            assert torch.equal(out, alpha)
            staged = torch.zeros((B, nrhs, npad), dtype=torch.float64, device=dev)
            staged[:, :, :n] = rhs
            solved = torch.empty_like(staged)
            cinv = timed(lambda: _lib.check(lib.sf_potrs_batch(
                D.ptr(A), npad, lda, npad * lda, B, 3, D.ptr(staged), nrhs, npad, nrhs * npad, D.ptr(solved), npad,
                nrhs * npad, D.stream_ptr(dev)), "sf_potrs_batch"), reps, back_to_back=True)
            print(f"N={N} B={B} nrhs={nrhs:2d}: sf_decompose_batch {whole:8.3f} ms per call, K_k alpha alone {matvec:8.3f} ms, "
                  f"sf_apply_batch(Cinv) {apply:8.3f} ms, C^-1 alone {cinv:8.3f} ms")
    do.release_workspace()
