"""Stand-alone timing of sf_potrs_batch (the Cholesky factor applied to right-hand sides) on synthetic SPD matrices.
    python tools/bench_potrs.py [reps] [B] [N ...]
Per op (L Z, L^-1 B, L^-T B, C^-1 B), N in {3008, 4096}, batch 128, nrhs in {1, 16}: ms per call and the achieved rate
against the bytes of L a call has to read, 8 N^2 / 2 per matrix, sweep and group of 16 right-hand sides."""
import torch
from _bench_common import arguments, dominant_matrices, factorised, timed

from starfish_amd import _device as D
from starfish_amd import _lib

reps, B, sizes = arguments(5)
lib = _lib.require_gpu()
dev = D.device_of()
s = D.stream_ptr(dev)
for N in sizes:
    lda = N + 16
    g = torch.Generator(device=dev).manual_seed(0)
    base, A = dominant_matrices(N, lda, B, dev, g)
    factorised(lib, A, N, lda, B, dev)
    for nrhs in (1, 16):
        rhs = torch.empty((B, nrhs, N), dtype=torch.float64, device=dev)
        rhs.normal_(generator=g)
        out = torch.empty_like(rhs)
        for name, op, sweeps in (("L", 0, 1), ("Linv", 1, 1), ("LinvT", 2, 1), ("Cinv", 3, 2)):
            ms = timed(lambda: _lib.check(lib.sf_potrs_batch(D.ptr(A), N, lda, N * lda, B, op, D.ptr(rhs), nrhs, N, nrhs * N,
                                                             D.ptr(out), N, nrhs * N, s), "sf_potrs_batch"),
                       reps, back_to_back=True)
            gb = sweeps * B * ((nrhs + 15) // 16) * 8.0 * N * N / 2 / 1e9
            print(f"N={N} B={B} nrhs={nrhs:2d} {name:5s}: {ms:8.3f} ms per call, {gb / ms * 1e3:7.1f} GB/s of L ({gb:.2f} GB)")
    x = out[0, 0]  # C^-1 b of the last call: residual against the matrix itself
    r = (base[:, :N] @ x - rhs[0, 0]).abs().max().item()
    print(f"N={N}: max |A x - b| = {r:.3g}")
    del A, rhs, out
