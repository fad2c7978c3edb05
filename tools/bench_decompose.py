"""Stand-alone timing of sf_decompose_batch (the residual split by covariance component) on synthetic orders.
    python tools/bench_decompose.py [reps] [B] [N ...]
Per N in {3008, 4096}, batch 128, nrhs in {1, 16}: ms per call of the whole sf_decompose_batch, of its last step alone (the
kernels of sf_cov_matvec.h, through sf_debug_decompose_matvec on the workspace the call left) and, beside them, of
sf_apply_batch with SF_APPLY_CINV (everything sf_decompose_batch does before that step) and of sf_potrs_batch with
SF_APPLY_CINV on synthetic factors of the same size (the C^-1 alone, the number tools/bench_potrs.py reports)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tests"))
import ctypes as C

import torch
from gpu_helpers import device_order, oracle_order, pack_rows

from starfish_amd import _device as D
from starfish_amd import _lib, synth

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
B = int(sys.argv[2]) if len(sys.argv) > 2 else 128
sizes = [int(a) for a in sys.argv[3:]] or [3008, 4096]
lib = _lib.require_gpu()


def timed(call):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for it in range(reps + 1):  # (the first call is not timed)
        if it == 1:
            t0.record()
        call()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


for N in sizes:
    o = synth.make_order(N=N, m=4, seed=5)
    do = device_order(oracle_order(o))
    md, rows = pack_rows(do, [synth.vector_to_oracle_params(p) for p in synth.walker_ball(o, B=B)])
    dev, n, npad, lda = do.dev, do.n, do.npad, do.lda
    with torch.cuda.device(dev):
        P = D.to_dev(rows, dev)
        g = torch.Generator(device=dev).manual_seed(0)
        # C^-1 alone: sf_potrs_batch on factors of the padded size, a diagonally dominant random symmetric matrix as
        # tools/bench_potrs.py builds it (the kernel's time does not depend on the values)
        base = torch.empty((npad, lda), dtype=torch.float64, device=dev)
        base.normal_(generator=g)
        base[:, :npad] = (base[:, :npad] + base[:, :npad].T) * 0.01
        base[:, :npad] += torch.eye(npad, dtype=torch.float64, device=dev) * 4.0
        A = base.unsqueeze(0).expand(B, npad, lda).contiguous()
        pinfo = torch.empty((B,), dtype=torch.int32, device=dev)
        pws = D.workspace(lib.sf_potrf_workspace_bytes(npad, B), dev)
        _lib.check(lib.sf_potrf_batch(D.ptr(A), npad, lda, npad * lda, B, D.ptr(pinfo), D.ptr(pws), pws.numel(),
                                      D.stream_ptr(dev)), "sf_potrf_batch")
        torch.cuda.synchronize()
        assert int(pinfo.abs().max()) == 0
        del pws, base
        for nrhs in (1, 16):
            rhs = torch.empty((B, nrhs, n), dtype=torch.float64, device=dev)
            rhs.normal_(generator=g)
            comp = D.empty((B, 3 + md.n_local, nrhs, n), dev)
            alpha, out = D.empty((B, nrhs, n), dev), D.empty((B, nrhs, n), dev)
            info = D.empty((B,), dev, torch.int32)
            ws = do._reserve(do.decompose_workspace_bytes(md, B, nrhs))
            whole = timed(lambda: do._call("decompose_batch", md, B, P, rhs, nrhs, n, nrhs * n, comp, alpha, None, info, ws=ws))
            assert int(info.abs().max()) == 0
            kept = comp.clone()
            matvec = timed(lambda: _lib.check(lib.sf_debug_decompose_matvec(
                do.ctx, C.byref(md), B, D.ptr(P), nrhs, D.ptr(comp), D.ptr(ws), ws.numel(), D.stream_ptr(dev)),
                "sf_debug_decompose_matvec"))
            assert torch.equal(comp, kept)  # the same bits as inside the whole call
            apply = timed(lambda: do._call("apply_batch", md, B, P, 3, rhs, nrhs, n, nrhs * n, out, None, info, ws=ws))
            assert torch.equal(out, alpha)
            staged = torch.zeros((B, nrhs, npad), dtype=torch.float64, device=dev)
            staged[:, :, :n] = rhs
            solved = torch.empty_like(staged)
            cinv = timed(lambda: _lib.check(lib.sf_potrs_batch(
                D.ptr(A), npad, lda, npad * lda, B, 3, D.ptr(staged), nrhs, npad, nrhs * npad, D.ptr(solved), npad,
                nrhs * npad, D.stream_ptr(dev)), "sf_potrs_batch"))
            print(f"N={N} B={B} nrhs={nrhs:2d}: sf_decompose_batch {whole:8.3f} ms per call, K_k alpha alone {matvec:8.3f} ms, "
                  f"sf_apply_batch(Cinv) {apply:8.3f} ms, C^-1 alone {cinv:8.3f} ms")
    do.release_workspace()
