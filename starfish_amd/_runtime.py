"""
What every device-side call shares: the status codes and their messages, the policy for the internal status, the PyTorch-ROCm
plumbing (tensors own the HBM buffers and the stream), workspaces and the chunk loop, the result buffers and the helpers of the
band solver's dispatchers.  Nothing here computes on the CPU; nothing here knows an order (``_device``) or a multi-order call
(``_multi``).
"""

import ctypes as C

import numpy as np

from . import _lib

INFO_MESSAGES = {
    -1: "Querying emulator outside of original parameter range.",
    -2: "vsini must be positive",
    -3: "emulator weight covariance is not positive definite",
    -4: "covariance support wider than the band half-width given to the banded solver",
    -5: "internal error: a bounded wait inside a persistent kernel gave up (banded sweep or dataflow Cholesky; "
        "no result of that call is valid -- is the GPU shared with another process?)",
    -6: "the log-likelihood evaluated to NaN (non-finite input or intermediate)",
}
APPLY_OPS = {"L": 0, "Linv": 1, "LinvT": 2, "Cinv": 3}  # SF_APPLY_* of include/starfish_amd.h
MEAN_GRAD_MAX_SLOTS = 16  # SF_MEAN_GRAD_MAX_SLOTS of include/starfish_amd.h
MAX_LOCAL = 32  # SF_MAX_LOCAL of csrc/sf_common.h: local kernels per model
LOCAL_SCAN_MAX_PATCH = 256  # SF_LOCAL_SCAN_MAX_PATCH of include/starfish_amd.h
INFO_BANDWIDTH = -4
INFO_INTERNAL = -5


def persistent_status(lib):
    """``sf_persistent_potrf_status`` as a dict (host memory of the library: read it after the stream was synchronised)."""
    buf = (C.c_longlong * 8)()
    _lib.check(lib.sf_persistent_potrf_status(buf), "sf_persistent_potrf_status")
    keys = ("aborted_launches", "reason", "workgroups_started", "grid", "wait_ticks", "tasks_completed",
            "launches", "enabled")
    return dict(zip(keys, (int(v) for v in buf)))


def recover_from_internal(lib, where, count, stacklevel=3):
    """A dense call came back with SF_INFO_INTERNAL: the persistent-kernel Cholesky gave a launch up and the whole batch
    is invalid (include/starfish_amd.h).  The reference would never turn that into a rejected proposal
    (spectrum_model.py:400 raises out of cho_factor), so: say so loudly -- with what the aborting workgroup recorded --,
    switch the PROCESS (all devices, all threads) to the launch sequences (no waits inside kernels) and let the caller
    re-run the batch."""
    import warnings

    st = persistent_status(lib)
    why = {1: "a wait between workgroups reached its 4-s bound",
           2: "no task of the launch completed for 25 ms"}.get(st["reason"], "no abort record")
    if st["grid"] and st["workgroups_started"] < st["grid"]:
        why += f"; only {st['workgroups_started']} of its {st['grid']} workgroups had started (grid not co-resident)"
    warnings.warn(
        f"{where}: internal status -5 for {int(count)} unit(s) -- the persistent-kernel Cholesky gave a launch up ({why}, "
        f"after {st['tasks_completed']} completed tasks): is this GPU shared with another process?  The kernel assumes "
        "one process per GPU.  It is now disabled for this whole process, on every device and thread "
        "(sf_persistent_potrf(0)), and the batch is re-run on the launch sequence.",
        RuntimeWarning,
        stacklevel=stacklevel,
    )
    lib.sf_persistent_potrf(0)


def retry_internal(lib, where, evaluate, count=None, stacklevel=4):
    """THE policy for SF_INFO_INTERNAL of the dense path.  ``evaluate(again) -> (result, info)`` runs the call and fetches
    its status codes; ``again`` is False for the first run and True for the one repeat after
    :func:`recover_from_internal` (never a silent -inf: warn, switch the persistent kernel off, evaluate again).  A -5 that
    survives the repeat is never an ordinary per-unit status -- no value of the call is valid: RuntimeError.  ``count``:
    the units the warning names (default: the -5 entries of ``info``); ``stacklevel``: the frame it is attributed to (default:
    the one that called our caller)."""
    result, info = evaluate(False)
    bad = int(np.count_nonzero(np.asarray(info) == INFO_INTERNAL))
    if not bad:
        return result
    recover_from_internal(lib, where, bad if count is None else count, stacklevel=stacklevel)
    result, info = evaluate(True)
    if np.any(np.asarray(info) == INFO_INTERNAL):
        raise RuntimeError(INFO_MESSAGES[INFO_INTERNAL])
    return result


def _torch():
    import torch

    return torch


def device_of(index=None):
    torch = _torch()
    if index is None:
        index = torch.cuda.current_device() if torch.cuda.is_available() else 0
    return torch.device("cuda", index)


def to_dev(arr, dev):
    torch = _torch()
    a = np.ascontiguousarray(np.asarray(arr, dtype=np.float64))
    return torch.from_numpy(a).to(dev)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def empty(shape, dev, dtype=None):
    torch = _torch()
    return torch.empty(shape, dtype=dtype or torch.float64, device=dev)


def current_stream(dev):
    return _torch().cuda.current_stream(dev)


def stream_ptr(dev):
    return C.c_void_p(current_stream(dev).cuda_stream)


def workspace(nbytes, dev):
    torch = _torch()
    return torch.empty(max(int(nbytes), 8), dtype=torch.uint8, device=dev)


def grow_workspace(slot, key, need, dev):
    """The byte buffer ``slot[key]``, grown to at least ``need`` bytes.  ``slot`` is the mapping that owns the buffer (an
    object's ``vars()`` or a dict): a buffer that is too small is dropped BEFORE the new one is allocated, which no
    reference held by a caller may prevent.  The buffer is handed to kernels on whatever stream is current (EchelleModel
    rotates orders over side streams), so that stream is recorded on it: the caching allocator then does not recycle a
    dropped buffer before the work queued on it has finished."""
    if slot[key] is None or slot[key].numel() < need:
        slot[key] = None
        slot[key] = workspace(need, dev)
    slot[key].record_stream(current_stream(dev))
    return slot[key]


HBM_RESERVE = 0.15  # share of the free HBM that the chunk sizes leave alone


def units_that_fit(dev, fixed_bytes, per_unit_bytes, held_bytes=0, limit=None):
    """How many units of ``per_unit_bytes`` workspace fit the free HBM of ``dev`` next to ``fixed_bytes``, at least 1, at
    most ``limit``.  ``held_bytes``: the buffer the caller is about to replace counts as free."""
    free, _total = _torch().cuda.mem_get_info(dev)
    cap = max(1, (int((free + held_bytes) * (1.0 - HBM_RESERVE)) - fixed_bytes) // per_unit_bytes)
    return cap if limit is None else min(cap, int(limit))


def run_chunked(lib, where, dev, slot, key, fixed_bytes, per_unit_bytes, limit, B, max_chunk, reserve, buffers, enqueue, download,
                count=None):
    """THE chunk loop of the batched calls: ``B`` units cut into chunks whose workspace fits the free HBM
    (:func:`units_that_fit` of ``fixed_bytes``, ``per_unit_bytes`` and ``limit``; the buffer ``slot[key]`` counts as free), at
    most ``max_chunk`` each; the results allocated (``buffers()``) and every chunk enqueued on ONE workspace
    (``reserve(units)``, which grows ``slot[key]``) with ``enqueue(bufs, lo, hi, ws)``; ``download(bufs)``, a dict with "info",
    returned; all of it once more if a status is SF_INFO_INTERNAL (:func:`retry_internal` with ``where`` and ``count``; its
    warning names the frame that called the caller of our caller)."""
    def run(again):
        held = slot[key].numel() if slot[key] is not None else 0
        chunk = min(B, max_chunk or B, units_that_fit(dev, fixed_bytes, per_unit_bytes, held, limit))
        bufs = buffers()
        ws = reserve(chunk)
        for lo in range(0, B, chunk):
            enqueue(bufs, lo, min(lo + chunk, B), ws)
        res = download(bufs)
        return res, res["info"]

    return retry_internal(lib, where, run, count=count, stacklevel=6)


def result_buffers(B, dev, resid_cols=None):
    """Device outputs of a likelihood call of ``B`` units: the (4, B) "quad" lnl / logdet / sqmah / log_scale (ONE
    device->host copy for the four double outputs), the int32 ``info`` and, asked for, the (B, resid_cols) residuals."""
    torch = _torch()
    return (empty((4, B), dev), empty((B,), dev, torch.int32),
            empty((B, resid_cols), dev) if resid_cols is not None else None)


def fetch_results(quad, info, resid=None):
    """Download what :func:`result_buffers` allocated: dict of numpy arrays lnl, logdet, sqmah, log_scale, info (+ resid)."""
    out = dict(zip(("lnl", "logdet", "sqmah", "log_scale"), quad.cpu().numpy()), info=info.cpu().numpy())
    if resid is not None:
        out["resid"] = resid.cpu().numpy()
    return out


def check_solver(solver, choices=("dense", "banded", "auto"), or_none=False):
    """``ValueError`` unless ``solver`` is one of ``choices`` (``or_none``: the message offers None too, which the caller has
    already replaced by its default)."""
    if solver not in choices:
        names = ["None"] * or_none + [repr(c) for c in choices]
        raise ValueError(f"solver must be {', '.join(names[:-1])} or {names[-1]}")


def refused_output(B, shapes):
    """What the band solver's dispatchers start from: every one of ``B`` walkers refused with INFO_BANDWIDTH -- ``lnl`` -inf,
    ``info`` -4, NaN in every other result (``shapes``: key -> trailing shape)."""
    out = dict(lnl=np.full(B, -np.inf))
    out.update({key: np.full((B,) + tuple(shape), np.nan) for key, shape in shapes.items()})
    out["info"] = np.full(B, INFO_BANDWIDTH, dtype=np.int32)
    return out


def finish_structured(out, fits, solver, dense):
    """THE tail of the band solver's dispatchers, once the banded groups' results are in ``out`` (:func:`refused_output`
    elsewhere).  An internal wait timeout of the sweep (-5, not expected: the bound keeps a logic error from hanging the GPU) is
    recomputed by the dense solver -- under "banded" too -- instead of silently turning into a rejected walker; under "auto" so
    are the walkers whose bound does not fit (``~fits``) and those the kernels flagged with -4.  ``dense(rest)`` gets their
    ascending indices, once, and returns the keys of ``out`` for them.  The warning names the caller's frame."""
    internal = out["info"] == INFO_INTERNAL
    if internal.any():
        import warnings

        warnings.warn(f"banded solver: internal status -5 for {int(internal.sum())} walker(s); recomputed densely",
                      RuntimeWarning, stacklevel=2)
    rest = np.nonzero(internal)[0]
    if solver == "auto":  # too wide for the banded kernels -> dense
        rest = np.nonzero(~fits | (out["info"] == INFO_BANDWIDTH) | internal)[0]
    if rest.size:
        got = dense(rest)
        for key in out:
            out[key][rest] = got[key]
    return out
