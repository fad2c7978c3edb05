"""Stand-alone timing of sf_potrs_batch (the Cholesky factor applied to right-hand sides) on synthetic SPD matrices.
    python tools/bench_potrs.py [reps] [B] [N ...]
Per op (L Z, L^-1 B, L^-T B, C^-1 B), N in {3008, 4096}, batch 128, nrhs in {1, 16}: ms per call and the achieved rate
against the bytes of L a call has to read, 8 N^2 / 2 per matrix, sweep and group of 16 right-hand sides."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import torch

from starfish_amd import _device as D
from starfish_amd import _lib

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
B = int(sys.argv[2]) if len(sys.argv) > 2 else 128
sizes = [int(a) for a in sys.argv[3:]] or [3008, 4096]
lib = _lib.require_gpu()
dev = D.device_of()
s = D.stream_ptr(dev)
for N in sizes:
    lda = N + 16
    # diagonally dominant random symmetric matrix generated on the device (plumbing only)
    g = torch.Generator(device=dev).manual_seed(0)
    base = torch.empty((N, lda), dtype=torch.float64, device=dev)
    base.normal_(generator=g)
    base[:, :N] = (base[:, :N] + base[:, :N].T) * 0.01
    base[:, :N] += torch.eye(N, dtype=torch.float64, device=dev) * 4.0
    A = base.unsqueeze(0).expand(B, N, lda).contiguous()
    info = torch.empty((B,), dtype=torch.int32, device=dev)
    ws = D.workspace(lib.sf_potrf_workspace_bytes(N, B), dev)
    _lib.check(lib.sf_potrf_batch(D.ptr(A), N, lda, N * lda, B, D.ptr(info), D.ptr(ws), ws.numel(), s), "sf_potrf_batch")
    torch.cuda.synchronize()
    assert int(info.abs().max()) == 0
    del ws
    for nrhs in (1, 16):
        rhs = torch.empty((B, nrhs, N), dtype=torch.float64, device=dev)
        rhs.normal_(generator=g)
        out = torch.empty_like(rhs)
        for name, op, sweeps in (("L", 0, 1), ("Linv", 1, 1), ("LinvT", 2, 1), ("Cinv", 3, 2)):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for it in range(reps + 1):  # (the first call is not timed)
                if it == 1:
                    t0.record()
                _lib.check(lib.sf_potrs_batch(D.ptr(A), N, lda, N * lda, B, op, D.ptr(rhs), nrhs, N, nrhs * N, D.ptr(out), N,
                                              nrhs * N, s), "sf_potrs_batch")
            t1.record()
            torch.cuda.synchronize()
            ms = t0.elapsed_time(t1) / reps
            gb = sweeps * B * ((nrhs + 15) // 16) * 8.0 * N * N / 2 / 1e9
            print(f"N={N} B={B} nrhs={nrhs:2d} {name:5s}: {ms:8.3f} ms per call, {gb / ms * 1e3:7.1f} GB/s of L ({gb:.2f} GB)")
    x = out[0, 0]  # C^-1 b of the last call: residual against the matrix itself
    r = (base[:, :N] @ x - rhs[0, 0]).abs().max().item()
    print(f"N={N}: max |A x - b| = {r:.3g}")
    del A, rhs, out
