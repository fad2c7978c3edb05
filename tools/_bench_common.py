"""What the stand-alone timers of the calls on the Cholesky factor share (bench_potrs.py, bench_decompose.py,
bench_pointwise.py, bench_gradient.py, bench_mean_gradient.py): the argv convention ``[reps] [B] [N ...]``, the event timing, the synthetic order with
its walkers and the synthetic factor."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tests"))
import torch

from starfish_amd import _device as D
from starfish_amd import _lib, synth


def arguments(default_reps):
    """reps, B, sizes of ``python tools/bench_*.py [reps] [B] [N ...]`` (B 128 and N 3008, 4096 if not given)."""
    argv = sys.argv
    return (int(argv[1]) if len(argv) > 1 else default_reps, int(argv[2]) if len(argv) > 2 else 128,
            [int(a) for a in argv[3:]] or [3008, 4096])


def timed(call, reps, before=None, back_to_back=False):
    """ms per call over ``reps`` calls (one more in front is not timed), every call between events of its own and
    synchronised.  ``before`` (untimed work, such as restoring an input) runs in front of every call.  ``back_to_back``: one
    pair of events around all the calls and no synchronisation between them."""
    total = 0.0
    for it in range(reps + 1):
        if before:
            before()
        if not back_to_back or it == 1:
            t0 = torch.cuda.Event(enable_timing=True)
            t0.record()
        call()
        if not back_to_back or it == reps:
            t1 = torch.cuda.Event(enable_timing=True)
            t1.record()
            torch.cuda.synchronize()
            if it:
                total += t0.elapsed_time(t1)
    return total / reps


def order_and_walkers(N, B):
    """The synthetic order of N pixels on the device and the parameters of B walkers around its truth."""
    from gpu_helpers import device_order, oracle_order

    o = synth.make_order(N=N, m=4, seed=5)
    return o, device_order(oracle_order(o)), [synth.vector_to_oracle_params(p) for p in synth.walker_ball(o, B=B)]


def dominant_matrices(n, lda, B, dev, g):
    """A diagonally dominant random symmetric matrix of order n and row stride lda, generated on the device (plumbing only;
    the kernels' time does not depend on the values), and B copies of it to factorise."""
    base = torch.empty((n, lda), dtype=torch.float64, device=dev)
    base.normal_(generator=g)
    base[:, :n] = (base[:, :n] + base[:, :n].T) * 0.01
    base[:, :n] += torch.eye(n, dtype=torch.float64, device=dev) * 4.0
    return base, base.unsqueeze(0).expand(B, n, lda).contiguous()


def potrf(lib, A, n, lda, B, info, ws, dev):
    _lib.check(lib.sf_potrf_batch(D.ptr(A), n, lda, n * lda, B, D.ptr(info), D.ptr(ws), ws.numel(), D.stream_ptr(dev)),
               "sf_potrf_batch")


def factorised(lib, A, n, lda, B, dev):
    """``A`` overwritten by its Cholesky factors (sf_potrf_batch)."""
    info = torch.empty((B,), dtype=torch.int32, device=dev)
    potrf(lib, A, n, lda, B, info, D.workspace(lib.sf_potrf_workspace_bytes(n, B), dev), dev)
    torch.cuda.synchronize()
    assert int(info.abs().max()) == 0
