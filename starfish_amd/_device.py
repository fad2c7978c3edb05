"""
Device-side plumbing: PyTorch-ROCm tensors own the HBM buffers and the stream, the arithmetic is done
by the HIP kernels behind the C-ABI (``_lib``).  Nothing here computes on the CPU.
"""

import ctypes as C

import numpy as np
# (at import, not inside factor_v11: there the import's cost -- a quarter of a second warm, more from a cold disk -- was part of
# a model's first likelihood call, which it outweighed several times)
from scipy.linalg import cho_solve, cholesky, solve_triangular

from . import _lib
from . import _rows as R

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
C_KMS = 2.99792458e5


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


def local_scan_patches(wave, cand):
    """The patch of every candidate of :meth:`DeviceOrder.local_scan` as the device finds it: ``cand`` (ncand, 2) = mu, sigma in
    km/s -> (lo, hi), the first and last pixel with ``c / mu |w - mu| <= 4 sigma (1 + 1e-9)`` on the sorted grid ``wave``;
    ``hi < lo`` (0, -1) where no pixel is in reach.  Pure host logic (numpy), the device's operations in the device's order."""
    w = np.asarray(wave, dtype=np.float64)
    cand = np.asarray(cand, dtype=np.float64).reshape(-1, 2)
    lo = np.zeros(len(cand), dtype=np.int64)
    hi = np.full(len(cand), -1, dtype=np.int64)
    n = w.size
    # (a sorted grid: the device's test is evaluated on a window around the interval a search gives, two pixels to spare)
    ordered = n > 1 and bool(np.all(np.diff(w) > 0))
    for q, (mu, sg) in enumerate(cand):
        r0 = 4 * sg
        a, b = 0, n
        if ordered and np.isfinite(mu) and np.isfinite(sg) and mu > 0:
            d = abs(r0) * mu / C_KMS
            a = max(int(np.searchsorted(w, mu - d, "left")) - 2, 0)
            b = min(int(np.searchsorted(w, mu + d, "right")) + 2, n)
        idx = np.nonzero(C_KMS / mu * np.abs(w[a:b] - mu) <= r0 * (1 + 1e-9))[0]
        if idx.size:
            lo[q], hi[q] = a + idx[0], a + idx[-1]
    return lo, hi


def band_halfwidth_bound(wave, rows, n_grid, has_global, n_local, n_cheb):
    """Per-walker upper bound on max|i-j| over the non-zero entries of the structured part of the
    covariance (global Matern taper r0 = 6 ls, Starfish/models/kernels.py:29; local patches r0 = 4 sigma,
    kernels.py:73), from host copies of the wavelength grid and of the C-ABI parameter rows
    (layout: :mod:`starfish_amd._rows`).
    Conservative: uses the smallest pixel spacing.  Pure host logic (numpy)."""
    w = np.asarray(wave, dtype=np.float64)
    rows = np.atleast_2d(np.asarray(rows, dtype=np.float64))
    big = np.iinfo(np.int32).max
    if w.size < 2 or not np.all(np.diff(w) > 0):
        return np.full(rows.shape[0], big, dtype=np.int64)
    hw = np.zeros(rows.shape[0])
    if has_global:
        # metric of the global kernel (kernels.py:27): r = c/2 |wi - wj| / (wi + wj), a quarter of the
        # velocity separation; r(i, i+d) >= d * dv * (1 - O(r0/c)) (slightly sub-additive)
        dv = float(np.min(C_KMS / 2 * (w[1:] - w[:-1]) / (w[1:] + w[:-1])))
        r0 = 6 * np.exp(rows[:, R.GLOBAL_LOG_LS])
        hw = np.maximum(hw, np.floor(r0 / dv * (1 + 4 * r0 / C_KMS + 1e-9)) + 1)
    lay = R.RowLayout(n_grid, R.model_desc(0, 0, 0, has_global, n_local, n_cheb))
    for k in range(n_local):
        mu, _log_amp, log_sigma = rows[:, lay.local_of(k)].T
        r0 = 4 * np.exp(log_sigma)
        # metric d_i = c/mu |w_i - mu| (kernels.py:69): patch = pixels with d_i <= r0; its extent in
        # pixels is at most 2 r0 / (smallest step of d), step of d >= (c/mu) * min(diff(w))
        step = C_KMS / np.abs(mu) * float(np.min(np.diff(w)))
        hw = np.maximum(hw, np.floor(2 * r0 / step * (1 + 1e-9)) + 1)
    return np.minimum(hw, big).astype(np.int64)


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


DIAGNOSE_WANTS = ("alpha", "cinv_diag", "cov_diag", "comp")


def diagnose_wants(want):
    """``want`` of :meth:`DeviceOrder.diagnose_banded` in the order of DIAGNOSE_WANTS, "alpha" always among them."""
    want = (want,) if isinstance(want, str) else tuple(want)
    unknown = [w for w in want if w not in DIAGNOSE_WANTS]
    if unknown:
        raise ValueError(f"want holds {unknown}: expected some of {list(DIAGNOSE_WANTS)}")
    return tuple(w for w in DIAGNOSE_WANTS if w == "alpha" or w in want)


def rhs_groups(nrhs, max_nrhs):
    """``nrhs`` right-hand sides cut into consecutive groups of at most ``max_nrhs`` (sf_diagnose_banded_max_nrhs), one call of
    the band solver each: the list of ``(lo, hi)``.  Pure host logic."""
    nrhs, max_nrhs = int(nrhs), int(max_nrhs)
    if nrhs < 1:
        raise ValueError("rhs holds no right-hand side")
    if max_nrhs < 1:
        raise ValueError("the band solver takes no right-hand side at this half-width")
    return [(lo, min(lo + max_nrhs, nrhs)) for lo in range(0, nrhs, max_nrhs)]


def factor_v11(v11, w_hat):
    """Init-time constants of the emulator conditional (the reference solves with the constant v11 on every call,
    emulator.py:387-388): Linv = inverse of the lower Cholesky factor of v11 and alpha = v11^-1 w_hat, by LAPACK on
    the host, once per hyper-parameter set -- every order context of the emulator receives the same arrays."""
    try:
        L = cholesky(np.asarray(v11, dtype=np.float64), lower=True)
    except np.linalg.LinAlgError as e:  # the library's documented status for this case (SF_INFO_EMULATOR_NOT_PD)
        raise np.linalg.LinAlgError(INFO_MESSAGES[-3]) from e
    linv = np.tril(solve_triangular(L, np.eye(L.shape[0]), lower=True))
    alpha = cho_solve((L, True), np.asarray(w_hat, dtype=np.float64))
    return np.ascontiguousarray(linv), np.ascontiguousarray(alpha)


def model_desc_key(md):
    """The fields of a ModelDesc as a hashable tuple (two orders may share a multi-order call only if equal)."""
    return tuple(int(getattr(md, name)) for name, _ in md._fields_)


class MultiPlan:
    """Device-resident state of a repeated multi-order evaluation (sf_loglike_multi_batch): parameter rows,
    outputs and workspace are allocated once; :meth:`enqueue` only launches.  ``orders`` are
    :class:`DeviceOrder` objects of ONE device, ``rows_list[i]`` the (B_i, stride) C-ABI rows of order i.
    ``md`` is one ModelDesc for every order (all rows of one layout), or a list with one ModelDesc per order
    (sf_loglike_multi_batch_md: orders with their own row layouts still share one batched Cholesky).
    Unit lists that do not fit the free HBM (or ``max_units``) are cut into several calls."""

    def __init__(self, orders, md, rows_list, max_units=None):
        torch = _torch()
        self.orders = list(orders)
        self.per_order = isinstance(md, (list, tuple))
        self.md = list(md) if self.per_order else md
        self.lib = orders[0].lib
        self.dev = orders[0].dev
        if any(o.dev != self.dev for o in orders):
            raise ValueError("multi-order call: all orders must live on the same device")
        if self.per_order:
            if len(self.md) != len(self.orders) or len(rows_list) != len(self.orders):
                raise ValueError(f"multi-order call: {len(self.md)} descriptors and {len(rows_list)} row blocks for "
                                 f"{len(self.orders)} orders")
            mds = self.md
        else:
            mds = [md] * len(self.orders)
        strides = [o.param_stride(m) for o, m in zip(orders, mds)]
        if not self.per_order and len(set(strides)) > 1:
            raise ValueError(f"multi-order call: one descriptor gives the orders row strides {sorted(set(strides))}")
        for want, r in zip(strides, rows_list):
            if int(r.shape[-1]) != want:
                raise ValueError(f"multi-order call: parameter rows of {int(r.shape[-1])} doubles do not match the "
                                 f"descriptor's stride {want} (orders with different descriptors need one descriptor "
                                 f"per order)")
        self.sizes = [int(np.atleast_2d(r).shape[0]) if not torch.is_tensor(r) else int(r.shape[0]) for r in rows_list]
        U = sum(self.sizes)
        with torch.cuda.device(self.dev):
            self.P = [r if torch.is_tensor(r) else to_dev(np.atleast_2d(r), self.dev) for r in rows_list]
            self.quad, self.info, _ = result_buffers(U, self.dev)
            # units that fit: the workspace is linear in the unit count up to the fixed Cholesky scratch.  With one
            # descriptor per order the largest estimate of any order counts (e.g. the only order whose descriptor
            # needs the broadening buffers: the call allocates them for all)
            fixed, per_unit = 0, 1
            for i in range(len(orders)) if self.per_order else (0,):
                one = _lib.Segment(orders[i].ctx, ptr(self.P[i]).value, 1, 0)
                desc = self._desc_array(mds[i:i + 1]) if self.per_order else C.byref(md)
                w1 = self._workspace_bytes(C.byref(one), 1, desc)
                one.B = 2
                w2 = self._workspace_bytes(C.byref(one), 1, desc)
                pu = max(w2 - w1, 1)
                per_unit, fixed = max(per_unit, pu), max(fixed, w1 - pu)
            lead = orders[0]
            held = lead._ws_multi.numel() if lead._ws_multi is not None else 0
            cap = units_that_fit(self.dev, fixed, per_unit, held, max_units or None)
            self.pieces, cur, cur_n = [], [], 0
            for i, n in enumerate(self.sizes):
                lo = 0
                while lo < n:
                    take = min(n - lo, cap - cur_n)
                    cur.append((i, lo, lo + take))
                    cur_n += take
                    lo += take
                    if cur_n == cap:
                        self.pieces.append(cur)
                        cur, cur_n = [], 0
            if cur:
                self.pieces.append(cur)
            offs = np.concatenate([[0], np.cumsum(self.sizes)])
            self.calls, need = [], 0
            for piece in self.pieces:
                segs = (_lib.Segment * len(piece))()
                for k, (i, lo, hi) in enumerate(piece):
                    segs[k] = _lib.Segment(orders[i].ctx, ptr(self.P[i][lo:hi]).value, hi - lo, 0)
                models = self._desc_array([mds[i] for i, _, _ in piece]) if self.per_order else C.byref(md)
                nb = self._workspace_bytes(segs, len(piece), models)
                if nb == 0:
                    _lib.check(-1, "sf_multi_workspace_bytes")
                need = max(need, nb)
                u0 = int(offs[piece[0][0]] + piece[0][1])  # the pieces of one call are contiguous in unit order
                self.calls.append((segs, len(piece), u0, sum(hi - lo for _, lo, hi in piece), models))
            self.ws = grow_workspace(vars(lead), "_ws_multi", need, self.dev)

    @staticmethod
    def _desc_array(mds):
        """``const sf_model_desc* const*`` of the given descriptors (the array keeps them alive)."""
        arr = (C.POINTER(_lib.ModelDesc) * len(mds))(*[C.pointer(m) for m in mds])
        arr._keep = mds
        return arr

    def _workspace_bytes(self, segs, nseg, models):
        fn = self.lib.sf_multi_workspace_bytes_md if self.per_order else self.lib.sf_multi_workspace_bytes
        return fn(segs, nseg, models)

    @property
    def units(self):
        return sum(self.sizes)

    def enqueue(self):
        """Launch only: results land in ``self.quad`` / ``self.info`` once the device's current stream is done."""
        torch = _torch()
        fn, name = ((self.lib.sf_loglike_multi_batch_md, "sf_loglike_multi_batch_md") if self.per_order
                    else (self.lib.sf_loglike_multi_batch, "sf_loglike_multi_batch"))
        with torch.cuda.device(self.dev):
            s = stream_ptr(self.dev)
            q = self.quad
            for segs, nseg, u0, n, models in self.calls:
                rc = fn(
                    segs, nseg, models, ptr(q[0][u0:u0 + n]), ptr(q[1][u0:u0 + n]), ptr(q[2][u0:u0 + n]),
                    ptr(q[3][u0:u0 + n]), ptr(self.info[u0:u0 + n]), ptr(self.ws), self.ws.numel(), s,
                )
                _lib.check(rc, name)

    def collect(self):
        def fetch(again):  # (the first run was enqueued by the caller)
            if again:
                self.enqueue()
            out = collect_multi(self.quad, self.info, self.sizes)
            return out, np.concatenate([o["info"] for o in out])

        return retry_internal(self.lib, "sf_loglike_multi_batch", fetch)


def loglike_multi(orders, md, rows_list, max_units=None, sync=True):
    """(order x walker) units of several orders of ONE device in one enqueue and one host synchronisation.
    ``md``: one ModelDesc shared by every order, or a list with one per order (see :class:`MultiPlan`).
    Returns a list of dicts (lnl, logdet, sqmah, log_scale, info) per order; with ``sync=False`` the
    un-synchronised :class:`MultiPlan` (callers overlapping several devices call ``plan.collect()`` later)."""
    plan = MultiPlan(orders, md, rows_list, max_units=max_units)
    plan.enqueue()
    return plan.collect() if sync else plan


class MultiGradPlan(MultiPlan):
    """Device-resident state of a repeated multi-order likelihood-and-gradient evaluation (sf_loglike_multi_grad_batch_md):
    one factorisation per (order x walker) unit gives the likelihood and the gradient in every requested slot.  ``mds``: one
    ModelDesc per order; ``requests[i]`` = ``(mean_columns, want_cov)``: the columns of order i's parameter row to
    differentiate in (as :meth:`DeviceOrder.loglike_mean_grad` takes them; may be empty) and whether its covariance slots
    (in :meth:`DeviceOrder.loglike_grad`'s order) are wanted.  The gradient row of a unit holds its order's mean slots in
    request order, then its covariance slots.  Buffers are allocated once; unit lists that do not fit the free HBM (or
    ``max_units``) are cut into several calls, a piece in which no order requests anything is a plain likelihood call."""

    def __init__(self, orders, mds, rows_list, requests, max_units=None):
        if len(requests) != len(orders):
            raise ValueError(f"multi-order gradient: {len(requests)} requests for {len(orders)} orders")
        self.requests = [([int(c) for c in cols], bool(cov)) for cols, cov in requests]
        self.slots = [len(cols) + (R.cov_grad_slots(md) if cov else 0) for (cols, cov), md in zip(self.requests, mds)]
        if not any(self.slots):
            raise ValueError("multi-order gradient: nothing to differentiate (no order requests a slot)")
        self.stride = max(self.slots)
        self._slot_arrays = [(C.c_int32 * max(len(cols), 1))(*cols) for cols, _ in self.requests]
        super().__init__(orders, list(mds), rows_list, max_units=max_units)
        with _torch().cuda.device(self.dev):
            self.grad = _torch().zeros((self.units, self.stride), dtype=_torch().float64, device=self.dev)

    def _requests_array(self, idxs):
        """``const sf_grad_request*`` of the given orders (the array keeps the column lists alive)."""
        arr = (_lib.GradRequest * len(idxs))()
        for k, i in enumerate(idxs):
            cols, cov = self.requests[i]
            arr[k] = _lib.GradRequest(self._slot_arrays[i], len(cols), int(cov))
        arr._keep = self._slot_arrays
        return arr

    def _orders_of(self, segs, nseg):
        """The orders of these segments, matched by context."""
        by_ctx = {int(o.ctx): i for i, o in enumerate(self.orders)}
        items = [segs[k] for k in range(nseg)] if isinstance(segs, C.Array) else [segs._obj]  # (an array, or byref of one)
        return [by_ctx[int(seg.ctx)] for seg in items]

    def _workspace_bytes(self, segs, nseg, models):
        """The gradient call's workspace for these segments."""
        idxs = self._orders_of(segs, nseg)
        if not any(self.slots[i] for i in idxs):
            return self.lib.sf_multi_workspace_bytes_md(segs, nseg, models)
        return self.lib.sf_multi_grad_workspace_bytes_md(segs, nseg, models, self._requests_array(idxs), self.stride)

    def enqueue(self):
        """Launch only: results land in ``self.quad`` (rows 0 lnl, 3 log_scale), ``self.info`` and ``self.grad`` once the
        device's current stream is done."""
        torch = _torch()
        with torch.cuda.device(self.dev):
            s = stream_ptr(self.dev)
            q = self.quad
            for (segs, nseg, u0, n, models), piece in zip(self.calls, self.pieces):
                idxs = [i for i, _, _ in piece]
                if not any(self.slots[i] for i in idxs):
                    rc = self.lib.sf_loglike_multi_batch_md(segs, nseg, models, ptr(q[0][u0:u0 + n]), None, None,
                                                            ptr(q[3][u0:u0 + n]), ptr(self.info[u0:u0 + n]), ptr(self.ws),
                                                            self.ws.numel(), s)
                    _lib.check(rc, "sf_loglike_multi_batch_md")
                    continue
                rc = self.lib.sf_loglike_multi_grad_batch_md(
                    segs, nseg, models, self._requests_array(idxs), ptr(q[0][u0:u0 + n]), ptr(q[3][u0:u0 + n]),
                    ptr(self.info[u0:u0 + n]), ptr(self.grad[u0:u0 + n]), self.stride, ptr(self.ws), self.ws.numel(), s)
                _lib.check(rc, "sf_loglike_multi_grad_batch_md")

    def collect(self):
        """Per order a dict of numpy arrays: lnl (B,), grad (B, slots of the order), log_scale (B,), info (B,); NaN rows
        where info != 0.  After SF_INFO_INTERNAL the whole batch is run once more (:func:`retry_internal`)."""
        def fetch(again):  # (the first run was enqueued by the caller)
            if again:
                self.enqueue()
            lnl, log_scale = self.quad[0].cpu().numpy(), self.quad[3].cpu().numpy()
            info, grad = self.info.cpu().numpy(), self.grad.cpu().numpy()
            ends = np.cumsum(self.sizes)
            out = [dict(lnl=lnl[hi - n:hi], grad=grad[hi - n:hi, :k], log_scale=log_scale[hi - n:hi], info=info[hi - n:hi])
                   for n, hi, k in zip(self.sizes, ends, self.slots)]
            return out, info

        return retry_internal(self.lib, "sf_loglike_multi_grad_batch_md", fetch)

    def reduce(self, sources):
        """The sum over the orders on the device (sf_multi_grad_reduce), of what a finished call left in the plan's buffers:
        ``sources[j]`` lists the ``(order, slot)`` pairs whose unit slots column j adds, ascending in the order.  Every
        order must have the same number of walkers W.  Returns numpy ``lnl (W,)``, ``grad (W, len(sources))``, ``info (W,)``."""
        torch = _torch()
        if len(set(self.sizes)) != 1:
            raise ValueError(f"sf_multi_grad_reduce: the orders have {sorted(set(self.sizes))} walkers")
        W, ncols = self.sizes[0], len(sources)
        col_ptr, col_src = column_map_csr(sources)
        with torch.cuda.device(self.dev):
            d_ptr, d_src = torch.from_numpy(col_ptr).to(self.dev), torch.from_numpy(col_src).to(self.dev)
            lnl, grad = empty((W,), self.dev), empty((W, max(ncols, 1)), self.dev)
            info = empty((W,), self.dev, torch.int32)
            rc = self.lib.sf_multi_grad_reduce(len(self.sizes), W, ptr(self.quad[0]), ptr(self.info), ptr(self.grad), self.stride,
                                               ptr(d_ptr), ptr(d_src), ncols, ptr(lnl), ptr(grad), max(ncols, 1), ptr(info),
                                               stream_ptr(self.dev))
            _lib.check(rc, "sf_multi_grad_reduce")
            return lnl.cpu().numpy(), grad.cpu().numpy()[:, :ncols], info.cpu().numpy()


def column_map_csr(sources):
    """``sources[j]`` = [(order, slot), ...] -> the int32 arrays ``col_ptr (ncols + 1,)`` and ``col_src (nnz, 2)`` of
    sf_multi_grad_reduce, the pairs of every column ascending in the order."""
    col_ptr = np.zeros(len(sources) + 1, dtype=np.int32)
    pairs = []
    for j, src in enumerate(sources):
        pairs += sorted((int(i), int(slot)) for i, slot in src)
        col_ptr[j + 1] = len(pairs)
    col_src = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    if not len(pairs):
        col_src = np.zeros((1, 2), dtype=np.int32)
    return col_ptr, np.ascontiguousarray(col_src)


def reduce_orders_host(lnl, info, grads, sources):
    """sf_multi_grad_reduce's rule on the host, for per-unit results that live on several devices: ``lnl``, ``info``
    (n_orders, W), ``grads[i]`` (W, slots of order i).  Every sum runs over the orders in ascending index, ``s = g0;
    s = s + g1; ...``; a column without a source is 0.0; ``info`` is the first non-zero code in that order, and a walker
    that has one gets ``-inf`` and a NaN row."""
    lnl, info = np.asarray(lnl, dtype=np.float64), np.asarray(info, dtype=np.int32)
    W = lnl.shape[1]
    total = lnl[0].copy()
    for i in range(1, lnl.shape[0]):
        total = total + lnl[i]
    code = np.zeros(W, dtype=np.int32)
    for i in range(info.shape[0]):
        code = np.where(code == 0, info[i], code)
    grad = np.zeros((W, len(sources)))
    for j, src in enumerate(sources):
        for q, (i, slot) in enumerate(sorted((int(i), int(slot)) for i, slot in src)):
            grad[:, j] = grads[i][:, slot] if q == 0 else grad[:, j] + grads[i][:, slot]
    bad = code != 0
    total[bad] = -np.inf
    grad[bad] = np.nan
    return total, grad, code


def loglike_multi_grad(orders, mds, rows_list, requests, max_units=None, sync=True):
    """The likelihood and its gradient for the (order x walker) units of several orders of ONE device, one factorisation per
    unit, in one enqueue and one host synchronisation (see :class:`MultiGradPlan` for ``mds`` and ``requests``).  Returns
    a list of dicts (lnl, grad, log_scale, info) per order; with ``sync=False`` the un-synchronised plan."""
    plan = MultiGradPlan(orders, mds, rows_list, requests, max_units=max_units)
    plan.enqueue()
    return plan.collect() if sync else plan


def banded_units(bounds, windows):
    """Which units of a multi-order gradient the band kernels take: ``bounds[i]`` (B_i,) the half-width bounds of order i's
    units, ``windows[i]`` its LDS window.  Returns ``fits``, one boolean array per order.  Pure host logic."""
    return [np.asarray(b) <= int(w) for b, w in zip(bounds, windows)]


def rerouted_units(fits, infos, solver):
    """The rule of :func:`finish_structured` per (order x walker) unit: ``infos[i]`` (B_i,) are the codes the band kernels
    left (INFO_BANDWIDTH where ``fits[i]`` is false: those units never ran).  Returns per order the ascending walker indices
    that go through the dense call: units with the internal status -5 under either solver; under "auto" also the units whose
    bound does not fit and those the kernels flagged -4.  Under "banded" the latter two stay refused.  Pure host logic."""
    check_solver(solver, ("banded", "auto"))
    out = []
    for f, info in zip(fits, infos):
        info = np.asarray(info)
        rest = info == INFO_INTERNAL
        if solver == "auto":
            rest = rest | ~np.asarray(f) | (info == INFO_BANDWIDTH)
        out.append(np.nonzero(rest)[0])
    return out


def merge_units(outs, rest, dense):
    """Put the dense results back by (order, walker): ``outs[i]`` the per-order dicts, ``rest[i]`` the walker indices of order
    i that were re-routed, ``dense`` the dicts of the dense call for the orders that have any, in order.  In place."""
    got = iter(dense)
    for out, idx in zip(outs, rest):
        if not len(idx):
            continue
        res = next(got)
        for key in out:
            out[key][idx] = res[key]
    return outs


class _BandedUnits(MultiGradPlan):
    """The device side of :class:`BandedMultiGradPlan`: the units the band kernels take, every segment with the half-width
    ``halfwidth`` (sf_loglike_banded_multi_grad_batch_md).  A piece of a cut unit list in which no order requests anything is
    the plain (dense) multi-order likelihood, as in :class:`MultiGradPlan`."""

    def __init__(self, orders, mds, rows_list, requests, halfwidth, max_units=None):
        self.halfwidth = int(halfwidth)
        super().__init__(orders, mds, rows_list, requests, max_units=max_units)

    def _halfwidths(self, nseg):
        return (C.c_int * nseg)(*([self.halfwidth] * nseg))

    def _workspace_bytes(self, segs, nseg, models):
        idxs = self._orders_of(segs, nseg)
        if not any(self.slots[i] for i in idxs):
            return self.lib.sf_multi_workspace_bytes_md(segs, nseg, models)
        return self.lib.sf_banded_multi_grad_workspace_bytes_md(segs, nseg, models, self._requests_array(idxs),
                                                                self._halfwidths(nseg), self.stride)

    def enqueue(self):
        torch = _torch()
        with torch.cuda.device(self.dev):
            s = stream_ptr(self.dev)
            q = self.quad
            for (segs, nseg, u0, n, models), piece in zip(self.calls, self.pieces):
                idxs = [i for i, _, _ in piece]
                if not any(self.slots[i] for i in idxs):
                    rc = self.lib.sf_loglike_multi_batch_md(segs, nseg, models, ptr(q[0][u0:u0 + n]), None, None,
                                                            ptr(q[3][u0:u0 + n]), ptr(self.info[u0:u0 + n]), ptr(self.ws),
                                                            self.ws.numel(), s)
                    _lib.check(rc, "sf_loglike_multi_batch_md")
                    continue
                rc = self.lib.sf_loglike_banded_multi_grad_batch_md(
                    segs, nseg, models, self._requests_array(idxs), self._halfwidths(nseg), ptr(q[0][u0:u0 + n]),
                    ptr(q[3][u0:u0 + n]), ptr(self.info[u0:u0 + n]), ptr(self.grad[u0:u0 + n]), self.stride, ptr(self.ws),
                    self.ws.numel(), s)
                _lib.check(rc, "sf_loglike_banded_multi_grad_batch_md")

    def collect(self):
        """As :meth:`MultiGradPlan.collect`, without its retry: the band sweep's internal status is recomputed densely per
        unit (:func:`rerouted_units`), not by a second run of the batch."""
        lnl, log_scale = self.quad[0].cpu().numpy(), self.quad[3].cpu().numpy()
        info, grad = self.info.cpu().numpy(), self.grad.cpu().numpy()
        ends = np.cumsum(self.sizes)
        return [dict(lnl=lnl[hi - n:hi], grad=grad[hi - n:hi, :k], log_scale=log_scale[hi - n:hi], info=info[hi - n:hi])
                for n, hi, k in zip(self.sizes, ends, self.slots)]


class BandedMultiGradPlan:
    """:class:`MultiGradPlan` on the band + Woodbury solver: the likelihood of every (order x walker) unit and its gradient
    in every requested slot from one keeping sweep per unit, all units of the device in one launch sequence
    (sf_loglike_banded_multi_grad_batch_md).  ``orders``, ``mds``, ``rows_list`` (host rows or tensors) and ``requests`` as
    for :class:`MultiGradPlan`; :meth:`collect` returns the same per-order dicts and :meth:`reduce` the same order sum.

    Every unit's half-width bound is computed on the host (:meth:`DeviceOrder.halfwidth_bound`); the units whose bound fits
    their order's LDS window form one group, and every segment is given the group's largest bound, so that a unit's bits do
    not depend on how the unit list is cut.  solver: "banded" -- the other units are refused with INFO_BANDWIDTH (-inf and a
    NaN row); "auto" -- they, the units the kernels flag -4 and units with the internal status -5 go through the dense
    :func:`loglike_multi_grad` with just those rows and are merged back by (order, walker).  Status -5 is recomputed densely
    under "banded" too, with the warning of :func:`finish_structured`."""

    def __init__(self, orders, mds, rows_list, requests, solver="banded", max_units=None):
        check_solver(solver, ("banded", "auto"))
        if len(requests) != len(orders):
            raise ValueError(f"multi-order gradient: {len(requests)} requests for {len(orders)} orders")
        torch = _torch()
        self.orders, self.mds, self.solver, self.max_units = list(orders), list(mds), solver, max_units
        self.requests = [([int(c) for c in cols], bool(cov)) for cols, cov in requests]
        self.slots = [len(cols) + (R.cov_grad_slots(md) if cov else 0) for (cols, cov), md in zip(self.requests, self.mds)]
        if not any(self.slots):
            raise ValueError("multi-order gradient: nothing to differentiate (no order requests a slot)")
        self.rows = [np.atleast_2d(r.cpu().numpy() if torch.is_tensor(r) else np.asarray(r, dtype=np.float64)) for r in rows_list]
        self.sizes = [int(r.shape[0]) for r in self.rows]
        self.bounds = [o.halfwidth_bound(md, r) for o, md, r in zip(self.orders, self.mds, self.rows)]
        self.fits = banded_units(self.bounds, self._windows())
        self.idx = [np.nonzero(f)[0] for f in self.fits]
        self.on_device = [i for i, idx in enumerate(self.idx) if idx.size]  # the orders that have a unit for the band kernels
        self.halfwidth = max((int(self.bounds[i][self.idx[i]].max()) for i in self.on_device), default=0)
        self.plan = None
        # (a group in which no order requests a slot has nothing for the gradient call: its units are refused or go dense)
        if self.on_device and any(self.slots[i] for i in self.on_device):
            self.plan = self._units([self.orders[i] for i in self.on_device], [self.mds[i] for i in self.on_device],
                                    [self.rows[i][self.idx[i]] for i in self.on_device],
                                    [self.requests[i] for i in self.on_device], self.halfwidth, max_units=max_units)
        else:
            self.fits = [np.zeros(n, dtype=bool) for n in self.sizes]
            self.idx, self.on_device = [np.zeros(0, dtype=np.int64)] * len(self.sizes), []
        self.complete = all(f.all() for f in self.fits)  # every unit is in the device plan, in unit order
        self.rerouted = None
        self._out = None

    # what a plan on other band kernels (:class:`BandedMultiFisherPlan`) states anew: the device side, the window its units must
    # fit, a refused order's results and the dense call of the re-routed units
    _units = _BandedUnits

    def _windows(self):
        """Per order, the largest half-width bound the band kernels of this plan take."""
        return [o.banded_window_halfwidth() for o in self.orders]

    def _refused(self, n, k):
        return refused_output(n, dict(grad=(k,), log_scale=()))

    def _dense(self, which, rest):
        """The dense results of the walkers ``rest[i]`` of the orders ``which``, one dict with the keys of :meth:`_refused` each."""
        sub = ([self.orders[i] for i in which], [self.mds[i] for i in which], [self.rows[i][rest[i]] for i in which])
        if any(self.slots[i] for i in which):
            dense = loglike_multi_grad(*sub, [self.requests[i] for i in which], max_units=self.max_units)
        else:
            dense = [dict(o, grad=np.zeros((len(o["lnl"]), 0))) for o in loglike_multi(*sub, max_units=self.max_units)]
        return [{key: d[key] for key in ("lnl", "grad", "log_scale", "info")} for d in dense]

    @property
    def units(self):
        return sum(self.sizes)

    def enqueue(self):
        """Launch only (no host synchronisation)."""
        if self.plan is not None:
            self.plan.enqueue()

    def collect(self):
        """Per order a dict of numpy arrays: lnl (B,), grad (B, slots of the order), log_scale (B,), info (B,), as
        :meth:`MultiGradPlan.collect`; refused units have ``-inf``, NaN and INFO_BANDWIDTH."""
        outs = []
        for n, k in zip(self.sizes, self.slots):
            outs.append(self._refused(n, k))
        if self.plan is not None:
            for i, got in zip(self.on_device, self.plan.collect()):
                for key, v in got.items():
                    outs[i][key][self.idx[i]] = v
        internal = sum(int(np.count_nonzero(o["info"] == INFO_INTERNAL)) for o in outs)
        if internal:
            import warnings

            warnings.warn(f"banded solver: internal status -5 for {internal} unit(s); recomputed densely", RuntimeWarning,
                          stacklevel=2)
        rest = rerouted_units(self.fits, [o["info"] for o in outs], self.solver)
        which = [i for i, idx in enumerate(rest) if len(idx)]
        self.rerouted = sum(len(idx) for idx in rest)
        if which:
            merge_units(outs, rest, self._dense(which, rest))
        self._out = outs
        return outs

    def reduce(self, sources):
        """The sum over the orders of a collected call, as :meth:`MultiGradPlan.reduce`: on the device
        (sf_multi_grad_reduce) when every unit ran on the band kernels and none was re-routed, else by
        :func:`reduce_orders_host` of the collected units -- the same rule, the same bits."""
        if self._out is None:
            raise RuntimeError("BandedMultiGradPlan.reduce: collect() first")
        if len(set(self.sizes)) != 1:
            raise ValueError(f"sf_multi_grad_reduce: the orders have {sorted(set(self.sizes))} walkers")
        if self.complete and not self.rerouted:
            return self.plan.reduce(sources)
        return reduce_orders_host(np.stack([o["lnl"] for o in self._out]), np.stack([o["info"] for o in self._out]),
                                  [o["grad"] for o in self._out], sources)


def loglike_banded_multi_grad(orders, mds, rows_list, requests, solver="banded", max_units=None, sync=True):
    """:func:`loglike_multi_grad` on the band solver (:class:`BandedMultiGradPlan`; ``solver``: "banded" or "auto")."""
    plan = BandedMultiGradPlan(orders, mds, rows_list, requests, solver=solver, max_units=max_units)
    plan.enqueue()
    return plan.collect() if sync else plan


class _BandedFisherUnits(_BandedUnits):
    """The device side of :class:`BandedMultiFisherPlan`: the units the band kernels take, every segment with the half-width
    ``halfwidth`` (sf_fisher_banded_multi_batch_md).  ``self.fisher``: (units, pmax, pmax), a unit's matrix in its leading
    p_i x p_i block."""

    def __init__(self, orders, mds, rows_list, requests, halfwidth, max_units=None):
        super().__init__(orders, mds, rows_list, requests, halfwidth, max_units=max_units)
        with _torch().cuda.device(self.dev):  # (the base class's gradient rows, units x pmax doubles, stay unused)
            self.fisher = empty((self.units, self.stride, self.stride), self.dev)

    def _workspace_bytes(self, segs, nseg, models):
        idxs = self._orders_of(segs, nseg)
        return self.lib.sf_fisher_banded_multi_workspace_bytes_md(segs, nseg, models, self._requests_array(idxs),
                                                                  self._halfwidths(nseg))

    def enqueue(self):
        torch = _torch()
        with torch.cuda.device(self.dev):
            s = stream_ptr(self.dev)
            q, ld = self.quad, self.stride
            for (segs, nseg, u0, n, models), piece in zip(self.calls, self.pieces):
                rc = self.lib.sf_fisher_banded_multi_batch_md(
                    segs, nseg, models, self._requests_array([i for i, _, _ in piece]), self._halfwidths(nseg),
                    ptr(q[0][u0:u0 + n]), ptr(q[3][u0:u0 + n]), ptr(self.info[u0:u0 + n]), ptr(self.fisher[u0:u0 + n]), ld, ld * ld,
                    ptr(self.ws), self.ws.numel(), s)
                _lib.check(rc, "sf_fisher_banded_multi_batch_md")

    def collect(self):
        """Per order a dict of numpy arrays: lnl (B,), fisher (B, p_i, p_i), info (B,).  No retry, as :meth:`_BandedUnits.collect`."""
        lnl, info, fisher = self.quad[0].cpu().numpy(), self.info.cpu().numpy(), self.fisher.cpu().numpy()
        ends = np.cumsum(self.sizes)
        return [dict(lnl=lnl[hi - n:hi], fisher=np.ascontiguousarray(fisher[hi - n:hi, :k, :k]), info=info[hi - n:hi])
                for n, hi, k in zip(self.sizes, ends, self.slots)]

    def reduce(self, sources):
        """The sum of the unit matrices over the orders on the device (sf_multi_fisher_reduce), of what a finished call left in
        the plan's buffers; ``sources`` as for :meth:`MultiGradPlan.reduce`.  Returns numpy ``lnl (W,)``,
        ``fisher (W, len(sources), len(sources))``, ``info (W,)``."""
        torch = _torch()
        if len(set(self.sizes)) != 1:
            raise ValueError(f"sf_multi_fisher_reduce: the orders have {sorted(set(self.sizes))} walkers")
        W, ncols, ld = self.sizes[0], len(sources), self.stride
        col_ptr, col_src = column_map_csr(sources)
        with torch.cuda.device(self.dev):
            d_ptr, d_src = torch.from_numpy(col_ptr).to(self.dev), torch.from_numpy(col_src).to(self.dev)
            lnl, fisher = empty((W,), self.dev), empty((W, max(ncols * ncols, 1)), self.dev)
            info = empty((W,), self.dev, torch.int32)
            rc = self.lib.sf_multi_fisher_reduce(len(self.sizes), W, ptr(self.quad[0]), ptr(self.info), ptr(self.fisher), ld, ld * ld,
                                                 ptr(d_ptr), ptr(d_src), ncols, ptr(lnl), ptr(fisher), max(ncols * ncols, 1),
                                                 ptr(info), stream_ptr(self.dev))
            _lib.check(rc, "sf_multi_fisher_reduce")
            return lnl.cpu().numpy(), fisher.cpu().numpy()[:, :ncols * ncols].reshape(W, ncols, ncols), info.cpu().numpy()


def reduce_fisher_host(lnl, info, fishers, sources):
    """sf_multi_fisher_reduce's rule on the host: ``lnl``, ``info`` (n_orders, W), ``fishers[i]`` (W, p_i, p_i) the unit matrices
    of order i, ``sources[j]`` the ``(order, slot)`` pairs of label j (at most one per order).  Entry ``(a, b)``, ``a >= b``, is
    the sum of ``fishers[i][:, slot_a, slot_b]`` over the orders i that appear in both labels' lists, ascending, ``s = f0; s = s +
    f1; ...``, exactly 0.0 without a common order, and is mirrored; ``lnl`` and ``info`` as :func:`reduce_orders_host`; a walker
    with a non-zero code gets ``-inf`` and a NaN matrix.  The same adds in the same order as the device: the same bits."""
    total, _none, code = reduce_orders_host(lnl, info, [], [])
    W, p = total.shape[0], len(sources)
    per_order = {}
    for j, src in enumerate(sources):
        for i, slot in src:
            labels, slots = per_order.setdefault(int(i), ([], []))
            if j in labels:
                raise ValueError(f"label {j} has two sources in order {int(i)}")
            labels.append(j)
            slots.append(int(slot))
    F, seen = np.zeros((W, p, p)), np.zeros((p, p), dtype=bool)
    for i in sorted(per_order):
        la, sl = (np.asarray(v, dtype=np.intp) for v in per_order[i])
        block = np.asarray(fishers[i], dtype=np.float64)[:, sl[:, None], sl[None, :]]
        ix = np.ix_(la, la)
        F[:, la[:, None], la[None, :]] = np.where(seen[ix], F[:, la[:, None], la[None, :]] + block, block)
        seen[ix] = True
    lower = np.tril_indices(p, -1)
    F[:, lower[1], lower[0]] = F[:, lower[0], lower[1]]
    bad = code != 0
    F[bad] = np.nan
    return total, F, code


class BandedMultiFisherPlan(BandedMultiGradPlan):
    """The Fisher information of the mean-flux parameters (:meth:`DeviceOrder.fisher_mean`) of every (order x walker) unit of
    ONE device from one sweep per unit, all units in one launch sequence (sf_fisher_banded_multi_batch_md).  ``columns[i]``: the
    columns of order i's parameter row (1 .. MEAN_GRAD_MAX_SLOTS).  The rules of :class:`BandedMultiGradPlan`, shared with it
    -- half-width bounds on the host, one group at the group's largest bound, :func:`rerouted_units`, :func:`merge_units` --
    with the window at the CALL's row count ``1 + m + max p_i``: the units that fit it go to the band kernels; under "banded" the
    others are refused (INFO_BANDWIDTH, NaN), under "auto" they, the units flagged -4 and those with status -5 go, per order,
    through the dense ``fisher_mean`` and are merged back by (order, walker); -5 is recomputed densely under "banded" too.
    :meth:`collect`: per order a dict lnl (B,), fisher (B, p_i, p_i), info (B,)."""

    _units = _BandedFisherUnits

    def __init__(self, orders, mds, rows_list, columns, solver="banded", max_units=None):
        columns = [[int(c) for c in cols] for cols in columns]
        for i, cols in enumerate(columns):
            if not 1 <= len(cols) <= MEAN_GRAD_MAX_SLOTS:
                raise ValueError(f"multi-order Fisher information: order {i} has {len(cols)} columns, not 1 .. {MEAN_GRAD_MAX_SLOTS}")
        self.pmax = max((len(cols) for cols in columns), default=0)
        super().__init__(orders, mds, rows_list, [(cols, False) for cols in columns], solver=solver, max_units=max_units)

    def _windows(self):
        """The bound of a unit fits where the window takes this plan's largest column count (sf_fisher_banded_max_slots)."""
        return [max((w for w in range(0, o.banded_window_halfwidth() + 1, 16) if o.fisher_banded_max_slots(w) >= self.pmax),
                    default=-1) for o in self.orders]

    def _refused(self, n, k):
        return refused_output(n, dict(fisher=(k, k)))

    def _dense(self, which, rest):
        return [self.orders[i].fisher_mean(self.mds[i], self.rows[i][rest[i]], self.requests[i][0], "dense", self.max_units)
                for i in which]

    def reduce(self, sources):
        """The sum of the unit matrices over the orders of a collected call: on the device (sf_multi_fisher_reduce) when every
        unit ran on the band kernels and none was re-routed, else by :func:`reduce_fisher_host` -- the same rule, the same bits."""
        if self._out is None:
            raise RuntimeError("BandedMultiFisherPlan.reduce: collect() first")
        if len(set(self.sizes)) != 1:
            raise ValueError(f"sf_multi_fisher_reduce: the orders have {sorted(set(self.sizes))} walkers")
        if self.complete and not self.rerouted:
            return self.plan.reduce(sources)
        return reduce_fisher_host(np.stack([o["lnl"] for o in self._out]), np.stack([o["info"] for o in self._out]),
                                  [o["fisher"] for o in self._out], sources)


def fisher_banded_multi(orders, mds, rows_list, columns, solver="banded", max_units=None, sync=True):
    """The likelihood and the Fisher information of the mean-flux parameters for the (order x walker) units of several orders of
    ONE device on the band solver (:class:`BandedMultiFisherPlan`; ``solver``: "banded" or "auto").  Returns its per-order
    dicts; with ``sync=False`` the un-synchronised plan."""
    plan = BandedMultiFisherPlan(orders, mds, rows_list, columns, solver=solver, max_units=max_units)
    plan.enqueue()
    return plan.collect() if sync else plan


def collect_multi(quad, info, sizes):
    host = fetch_results(quad, info)
    ends = np.cumsum(sizes)
    return [{key: v[hi - n:hi] for key, v in host.items()} for n, hi in zip(sizes, ends)]


class DeviceOrder:
    """One ``sf_ctx``: the static data of an order + emulator resident in HBM, and the batched calls."""

    def __init__(
        self,
        wave,
        flux,
        sigma,
        min_dv_wave,
        bulk_fluxes,
        grid_points,
        variances,
        lengthscales,
        v11,
        w_hat,
        device=None,
        emu_factor=None,
    ):
        """``emu_factor``: optional ``(Linv, alpha)`` of the constant v11 (see :func:`factor_v11`), shared by all
        orders of one emulator; without it the library factors v11 itself (scalar host code)."""
        self.lib = _lib.require_gpu()
        torch = _torch()
        self.dev = device_of(device)
        f8 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64))  # noqa: E731
        self._keep = [
            f8(wave),
            f8(flux),
            f8(sigma),
            f8(min_dv_wave),
            f8(bulk_fluxes),
            f8(grid_points),
            f8(variances),
            f8(lengthscales),
            f8(v11),
            f8(w_hat),
        ]
        w, fl, sg, mdw, bulk, grid, var, ls, v11a, wh = self._keep
        self.n = int(w.shape[0])
        self.nf = int(mdw.shape[0])
        self.m = int(var.shape[0])
        self.M, self.P = (int(grid.shape[0]), int(grid.shape[1]))
        if self.n:
            assert bulk.shape == (self.m + 2, self.nf), bulk.shape
        assert v11a.shape == (self.m * self.M,) * 2
        d = _lib.OrderDesc()
        d.n, d.nf, d.m, d.n_grid, d.M = self.n, self.nf, self.m, self.P, self.M
        d.wave, d.flux, d.sigma = map(_lib.as_double_p, (w, fl, sg))
        d.min_dv_wave, d.bulk_fluxes = _lib.as_double_p(mdw), _lib.as_double_p(bulk)
        d.grid_points, d.variances = _lib.as_double_p(grid), _lib.as_double_p(var)
        d.lengthscales, d.v11, d.w_hat = map(_lib.as_double_p, (ls, v11a, wh))
        if emu_factor is not None:
            linv, alpha = f8(emu_factor[0]), f8(emu_factor[1])
            assert linv.shape == v11a.shape and alpha.shape == (v11a.shape[0],)
            self._keep += [linv, alpha]
            d.linv, d.alpha = _lib.as_double_p(linv), _lib.as_double_p(alpha)
        err = C.c_int(0)
        with torch.cuda.device(self.dev):
            self.ctx = self.lib.sf_ctx_create(C.byref(d), self.dev.index or 0, C.byref(err))
        if not self.ctx:
            _lib.check(err.value or -1, "sf_ctx_create")
        self.npad = self.lib.sf_ctx_npad(self.ctx)
        self.lda = self.lib.sf_ctx_lda(self.ctx)
        self._ws = None
        self._ws_multi = None  # workspace of loglike_multi calls led by this order

    def __del__(self):
        try:
            if getattr(self, "ctx", None):
                self.lib.sf_ctx_destroy(self.ctx)
                self.ctx = None
        except Exception:
            pass

    # ------------------------------------------------------------------ helpers
    def model_desc(self, *args, **kwargs):
        return R.model_desc(*args, **kwargs)

    def param_stride(self, md):
        stride = self.lib.sf_param_stride(self.ctx, C.byref(md))
        if stride < 0:  # a model the library does not take (e.g. more local kernels than SF_MAX_LOCAL): say why
            _lib.check(stride, "sf_param_stride")
        return stride

    def _size_query(self, call, md, *counts):
        return getattr(self.lib, f"sf_{call}workspace_bytes")(self.ctx, C.byref(md), *(int(v) for v in counts))

    def workspace_bytes(self, md, B):
        return self._size_query("", md, B)

    def max_batch(self, md):
        """Largest batch whose workspace fits the free HBM (leaving a safety margin)."""
        held = self._ws.numel() if self._ws is not None else 0
        return units_that_fit(self.dev, 0, max(self.workspace_bytes(md, 1), 1), held)

    def _reserve(self, need):
        """The order's workspace, grown to ``need`` bytes (:func:`grow_workspace`)."""
        return grow_workspace(vars(self), "_ws", need, self.dev)

    def _call(self, name, md, B, P, *args, ws=None):
        """Enqueue ``sf_<name>(ctx, &md, B, P, *args, ws, ws_bytes, stream)`` on the current stream and check its return
        code.  ``args``: integers and ctypes arrays (host arguments) as they are, tensors (or None) as their device pointers; ``ws``: the order's workspace
        sized for ``(md, B)`` unless the caller reserved another (the banded solver's)."""
        if ws is None:
            ws = self._work(md, B)
        args = [a if isinstance(a, (int, np.integer, C.Array)) else ptr(a) for a in args]
        rc = getattr(self.lib, "sf_" + name)(self.ctx, C.byref(md), B, ptr(P), *args, ptr(ws), ws.numel(),
                                             stream_ptr(self.dev))
        _lib.check(rc, "sf_" + name)

    def _work(self, md, B):
        return self._reserve(self.workspace_bytes(md, B))

    def release_workspace(self):
        self._ws = None
        self._ws_multi = None

    # ------------------------------------------------------------------ structure-exploiting solver
    def banded_window_halfwidth(self):
        """Half-widths up to this value use the LDS-window sweep; wider ones the in-place HBM/L2 kernel."""
        return int(self.lib.sf_banded_window_halfwidth(self.ctx)) if self.n else -1

    def banded_max_halfwidth(self):
        """Largest band half-width (pixels) sf_loglike_banded_batch accepts for this order; -1 = unusable."""
        return int(self.lib.sf_banded_max_halfwidth(self.ctx)) if self.n else -1

    def halfwidth_bound(self, md, rows):
        """Per-walker upper bound (pixels) on the support of the structured part of the covariance."""
        return band_halfwidth_bound(self._keep[0], rows, self.P, bool(md.has_global), int(md.n_local), int(md.n_cheb))

    def banded_workspace_bytes(self, md, B, halfwidth):
        return self._size_query("banded_", md, B, halfwidth)

    def _work_banded(self, md, B, halfwidth):
        return self._reserve(self.banded_workspace_bytes(md, B, halfwidth))

    def loglike_banded_device(self, md, P_dev, halfwidth, out_lnl, info=None, logdet=None, sqmah=None,
                              resid=None, log_scale=None):
        """Enqueue-only banded + rank-m solve (sf_loglike_banded_batch); device tensors in/out."""
        B = int(P_dev.shape[0])
        self._call("loglike_banded_batch", md, B, P_dev, int(halfwidth), out_lnl, logdet, sqmah, resid, log_scale, info,
                   ws=self._work_banded(md, B, halfwidth))

    # ------------------------------------------------------------------ batched calls
    def _host_rows_and_bound(self, md, params):
        """Parameter rows (numpy or tensor) as a (B, stride) float64 host array, and :meth:`halfwidth_bound` of them."""
        rows = params.cpu().numpy() if _torch().is_tensor(params) else np.asarray(params, dtype=np.float64)
        rows = np.atleast_2d(rows)
        return rows, self.halfwidth_bound(md, rows)

    def _rows(self, params):
        """Parameter rows ((B, stride) float64, numpy or tensor) on the order's device."""
        return params if _torch().is_tensor(params) else to_dev(params, self.dev)

    def _run_chunked(self, name, md, P, max_chunk, workspace_bytes, buffers, args, download):
        """:func:`run_chunked` for the dense calls ``sf_<name>(ctx, &md, B, P, *args(bufs, lo, hi), ws, ...)`` on the order's
        workspace: nothing fixed, ``workspace_bytes(1)`` per walker."""
        def enqueue(bufs, lo, hi, ws):
            self._call(name, md, hi - lo, P[lo:hi], *args(bufs, lo, hi), ws=ws)

        return run_chunked(self.lib, "sf_" + name, self.dev, vars(self), "_ws", 0, max(workspace_bytes(1), 1), None,
                           int(P.shape[0]), max_chunk, lambda units: self._reserve(workspace_bytes(units)), buffers, enqueue,
                           download)

    def loglike(self, md, params, want_resid=False, max_chunk=None, solver="dense"):
        """params: (B, stride) float64 (numpy or cuda tensor) in the C-ABI row layout.
        Returns dict of numpy arrays: lnl, logdet, sqmah, log_scale, info (+ resid).

        solver: "dense"  -- the reference's algorithm, batched N x N Cholesky (sf_loglike_batch);
                "banded" -- band + rank-m Woodbury solve (sf_loglike_banded_batch); walkers whose
                            covariance support exceeds the window come back with info = -4;
                "auto"   -- banded for the walkers whose half-width bound fits, dense for the rest."""
        torch = _torch()
        check_solver(solver)
        if solver != "dense":
            return self._loglike_structured(md, params, want_resid, max_chunk, solver)
        with torch.cuda.device(self.dev):
            P = self._rows(params)

            def args(bufs, lo, hi):
                quad, info, resid = bufs
                return (quad[0][lo:hi], quad[1][lo:hi], quad[2][lo:hi], resid[lo:hi] if want_resid else None, quad[3][lo:hi],
                        info[lo:hi])

            return self._run_chunked("loglike_batch", md, P, max_chunk, lambda units: self.workspace_bytes(md, units),
                                     lambda: result_buffers(int(P.shape[0]), self.dev, self.n if want_resid else None), args,
                                     lambda bufs: fetch_results(*bufs))

    def _loglike_structured(self, md, params, want_resid, max_chunk, solver):
        return self.structured_collect(md, self.structured_enqueue(md, params, want_resid, max_chunk), solver)

    def structured_enqueue(self, md, params, want_resid=False, max_chunk=None):
        """First half of the structure-exploiting evaluation: group the walkers by covariance support and ENQUEUE the
        banded calls on the current stream -- no host synchronisation.  :meth:`structured_collect` (after the stream
        is done) fetches the results; callers with several orders enqueue them all first (EchelleModel)."""
        torch = _torch()
        rows, hw = self._host_rows_and_bound(md, params)
        fits = hw <= self.banded_max_halfwidth()  # (solver="banded": the walkers that do not fit are reported with info = -4)
        shapes = dict(logdet=(), sqmah=(), log_scale=(), **({"resid": (self.n,)} if want_resid else {}))
        out = refused_output(rows.shape[0], shapes)
        groups = []
        # two groups: the cost of the wide-band factorisation grows with the half-width, so the walkers that fit the
        # LDS window are not dragged along with the wide ones
        wwin = self.banded_window_halfwidth()
        parts = [idx for idx in (np.nonzero(fits & (hw <= wwin))[0], np.nonzero(fits & (hw > wwin))[0]) if idx.size]
        # ONE allocation for both groups, made before anything is enqueued: the second group must not drop the
        # buffer the first group's kernels are still queued on
        if parts:
            self._reserve(max(self.banded_workspace_bytes(md, min(idx.size, max_chunk or idx.size), int(hw[idx].max()))
                              for idx in parts))
        for idx in parts:
            W = int(hw[idx].max())
            with torch.cuda.device(self.dev):
                P = to_dev(rows[idx], self.dev)
                nb = idx.size
                quad, info, resid = result_buffers(nb, self.dev, self.n if want_resid else None)
                lnl, logdet, sqmah, lsc = quad[0], quad[1], quad[2], quad[3]
                chunk = min(nb, max_chunk or nb)
                for lo in range(0, nb, chunk):
                    hi = min(lo + chunk, nb)
                    self.loglike_banded_device(
                        md, P[lo:hi], W, lnl[lo:hi], info[lo:hi], logdet[lo:hi], sqmah[lo:hi],
                        resid[lo:hi] if want_resid else None, lsc[lo:hi],
                    )
                groups.append((idx, quad, info, resid, P))
        return dict(out=out, groups=groups, fits=fits, rows=rows, want_resid=want_resid, max_chunk=max_chunk)

    def structured_collect(self, md, pend, solver):
        out, rows = pend["out"], pend["rows"]
        for idx, quad, info, resid, _ in pend["groups"]:
            for key, v in fetch_results(quad, info, resid).items():
                out[key][idx] = v
        return finish_structured(out, pend["fits"], solver, lambda rest: self.loglike(
            md, rows[rest], want_resid=pend["want_resid"], max_chunk=pend["max_chunk"], solver="dense"))

    def apply_workspace_bytes(self, md, B, nrhs):
        return self._size_query("apply_", md, B, nrhs)

    def decompose_workspace_bytes(self, md, B, nrhs):
        return self._size_query("decompose_", md, B, nrhs)

    def pointwise_workspace_bytes(self, md, B, nrhs):
        return self._size_query("pointwise_", md, B, nrhs)

    def loglike_grad_workspace_bytes(self, md, B):
        return self._size_query("loglike_grad_", md, B)

    def _rhs_on_device(self, rhs, B):
        """``rhs`` of :meth:`apply` / :meth:`decompose` as (contiguous device tensor or None, nrhs, per_walker)."""
        torch = _torch()
        if rhs is None:
            return None, 1, False
        R = rhs if torch.is_tensor(rhs) else to_dev(rhs, self.dev)
        if R.dim() not in (2, 3) or int(R.shape[-1]) != self.n or (R.dim() == 3 and int(R.shape[0]) != B):
            raise ValueError(f"rhs of shape {tuple(R.shape)}: expected (nrhs, {self.n}) or ({B}, nrhs, {self.n})")
        nrhs = int(R.shape[-2])
        if nrhs < 1:
            raise ValueError("rhs holds no right-hand side")
        return R.contiguous(), nrhs, R.dim() == 3

    def _outputs(self, B, outputs, want_flux):
        """``buffers`` and ``download`` of :meth:`_run_chunked` for the calls that apply the factor: ``bufs`` = (the (B, ...)
        double results in the order of ``outputs``, key -> trailing shape; the int32 status; the (B, n) flux or None)."""
        torch = _torch()

        def buffers():
            return ([empty((B,) + tuple(shape), self.dev) for shape in outputs.values()], empty((B,), self.dev, torch.int32),
                    empty((B, self.n), self.dev) if want_flux else None)

        def download(bufs):
            outs, info, flux = bufs
            res = {key: o.cpu().numpy() for key, o in zip(outputs, outs)}
            res["info"] = info.cpu().numpy()
            if want_flux:
                res["flux"] = flux.cpu().numpy()
            return res

        return buffers, download

    def _run_applied(self, name, md, params, rhs, outputs, want_flux, max_chunk, workspace_bytes, lead=()):
        """:meth:`_run_chunked` for ``sf_<name>(ctx, &md, B, P, *lead, rhs, nrhs, ldr, rhs_stride, *outputs, flux, info, ws,
        ...)``.  ``outputs(nrhs)``: key -> trailing shape of a (B, ...) double result."""
        with _torch().cuda.device(self.dev):
            P = self._rows(params)
            R, nrhs, per_walker = self._rhs_on_device(rhs, int(P.shape[0]))
            buffers, download = self._outputs(int(P.shape[0]), outputs(nrhs), want_flux)

            def args(bufs, lo, hi):
                outs, info, flux = bufs
                return (*lead, R[lo:hi] if per_walker else R, nrhs, self.n, nrhs * self.n if per_walker else 0,
                        *[o[lo:hi] for o in outs], flux[lo:hi] if want_flux else None, info[lo:hi])

            return self._run_chunked(name, md, P, max_chunk, lambda units: workspace_bytes(md, units, nrhs), buffers, args,
                                     download)

    def apply(self, md, params, op, rhs=None, want_flux=False, max_chunk=None, solver="dense"):
        """The Cholesky factor of every walker's covariance matrix applied to right-hand sides (sf_apply_batch): ``op`` is
        "L" (L z), "Linv" (L^-1 b), "LinvT" (L^-T b) or "Cinv" (C^-1 b = cho_solve), or its SF_APPLY_* number.
        params: (B, stride) rows as for :meth:`loglike`.  rhs: None (each walker's own residual), (nrhs, n) shared by all
        walkers or (B, nrhs, n).  Returns dict of numpy arrays: out (B, nrhs, n), NaN for walkers with info != 0, info
        (the codes of :meth:`loglike`) and, asked for, flux (B, n).

        solver: "dense" -- the dense factor (sf_apply_batch); "banded" / "auto" -- :meth:`diagnose_banded`, for "Cinv" only:
        the band solver has no triangular factor of C, so "L", "Linv" and "LinvT" with it are a ``ValueError``."""
        code = APPLY_OPS[op] if isinstance(op, str) else int(op)
        check_solver(solver)
        if solver != "dense":
            if code != APPLY_OPS["Cinv"]:
                raise ValueError(f'op {op!r} needs the dense factor: solver={solver!r} has no triangular factor of C ("Cinv" only)')
            res = self.diagnose_banded(md, params, rhs, ("alpha",), want_flux=want_flux, max_chunk=max_chunk, solver=solver)
            res["out"] = res.pop("alpha")
            return res
        return self._run_applied("apply_batch", md, params, rhs, lambda nrhs: {"out": (nrhs, self.n)}, want_flux, max_chunk,
                                 self.apply_workspace_bytes, lead=(code,))

    def decompose(self, md, params, rhs=None, want_flux=False, max_chunk=None, solver="dense"):
        """The right-hand sides split by covariance component (sf_decompose_batch): ``alpha = C^-1 rhs`` as :meth:`apply`
        with "Cinv" gives it, and ``comp[b, k] = K_k alpha`` for k = 0 emulator, 1 noise (jitter included), 2 global (zeros
        without one), 3 + j local kernel j.  params, rhs: as for :meth:`apply`.  Returns dict of numpy arrays: comp
        (B, 3 + n_local, nrhs, n), alpha (B, nrhs, n), info and, asked for, flux (B, n); NaN rows where info != 0.
        Chunked and retried like :meth:`apply`.  solver: "dense" (sf_decompose_batch), or "banded" / "auto":
        :meth:`diagnose_banded`."""
        check_solver(solver)
        if solver != "dense":
            return self.diagnose_banded(md, params, rhs, ("alpha", "comp"), want_flux=want_flux, max_chunk=max_chunk, solver=solver)
        outputs = lambda nrhs: {"comp": (3 + int(md.n_local), nrhs, self.n), "alpha": (nrhs, self.n)}  # noqa: E731
        return self._run_applied("decompose_batch", md, params, rhs, outputs, want_flux, max_chunk,
                                 self.decompose_workspace_bytes)

    def pointwise(self, md, params, rhs=None, want_flux=False, max_chunk=None, solver="dense"):
        """What the per-pixel leave-one-out diagnostics need (sf_pointwise_batch): ``alpha = C^-1 rhs`` as :meth:`apply`
        with "Cinv" gives it, ``cinv_diag = diag(C^-1)`` and ``cov_diag = diag(C)``, jitter included, as it was factorised.
        params, rhs: as for :meth:`apply`.  Returns dict of numpy arrays: alpha (B, nrhs, n), cinv_diag (B, n), cov_diag
        (B, n), info and, asked for, flux (B, n); NaN rows where info != 0.  Chunked and retried like :meth:`apply`.
        solver: "dense" (sf_pointwise_batch), or "banded" / "auto": :meth:`diagnose_banded`."""
        check_solver(solver)
        if solver != "dense":
            return self.diagnose_banded(md, params, rhs, ("alpha", "cinv_diag", "cov_diag"), want_flux=want_flux,
                                        max_chunk=max_chunk, solver=solver)
        outputs = lambda nrhs: {"alpha": (nrhs, self.n), "cinv_diag": (self.n,), "cov_diag": (self.n,)}  # noqa: E731
        return self._run_applied("pointwise_batch", md, params, rhs, outputs, want_flux, max_chunk,
                                 self.pointwise_workspace_bytes)

    # ------------------------------------------------------------------ residual diagnostics on the band solver
    def diagnose_banded_max_nrhs(self, halfwidth):
        """Most right-hand sides one sf_diagnose_banded_batch call takes at this half-width (0: none)."""
        return max(int(self.lib.sf_diagnose_banded_max_nrhs(self.ctx, int(halfwidth))), 0) if self.n else 0

    def diagnose_banded_workspace_bytes(self, md, B, halfwidth, nrhs, want_cinv_diag=False, want_comp=False):
        return self._size_query("diagnose_banded_", md, B, halfwidth, nrhs, int(bool(want_cinv_diag)), int(bool(want_comp)))

    def _diagnose_shapes(self, md, want, nrhs, want_flux):
        """key -> trailing shape of the results of :meth:`diagnose_banded` (without info)."""
        shapes = {"alpha": (nrhs, self.n), "cinv_diag": (self.n,), "cov_diag": (self.n,),
                  "comp": (3 + int(md.n_local), nrhs, self.n)}
        shapes = {key: shapes[key] for key in want}
        if want_flux:
            shapes["flux"] = (self.n,)
        return shapes

    def _diagnose_banded_group(self, md, rows, W, R, per_walker, cols, want, want_flux, max_chunk):
        """One sf_diagnose_banded_batch per chunk of ``rows`` at the half-width ``W`` for the right-hand sides ``cols`` =
        (lo, hi) of ``R`` (None: the walkers' own residuals): the dict of the results in ``want`` (+ flux, info)."""
        torch = _torch()
        lo_r, hi_r = cols
        k = hi_r - lo_r
        with torch.cuda.device(self.dev):
            P = self._rows(rows)
            B = int(P.shape[0])
            buffers, download = self._outputs(B, self._diagnose_shapes(md, want, k, False), want_flux)
            ktot = int(R.shape[-2]) if R is not None else 1

            def args(bufs, lo, hi):
                outs, info, flux = bufs
                by_key = {key: o[lo:hi] for key, o in zip(want, outs)}
                rhs = None if R is None else (R[lo:hi, lo_r:hi_r] if per_walker else R[lo_r:hi_r])
                return (W, rhs, k, self.n, ktot * self.n if per_walker else 0, by_key["alpha"], by_key.get("cinv_diag"),
                        by_key.get("cov_diag"), by_key.get("comp"), flux[lo:hi] if want_flux else None, info[lo:hi])

            size = lambda units: self.diagnose_banded_workspace_bytes(md, units, W, k, "cinv_diag" in want, "comp" in want)  # noqa: E731
            return self._run_chunked("diagnose_banded_batch", md, P, max_chunk, size, buffers, args, download)

    def _diagnose_dense(self, md, rows, rhs, want, want_flux, max_chunk):
        """The results of :meth:`diagnose_banded` from the dense calls, each as its own call gives it."""
        res = {}
        if "comp" in want:
            res.update(self.decompose(md, rows, rhs, want_flux=want_flux, max_chunk=max_chunk))
        if "cinv_diag" in want or "cov_diag" in want:
            res.update(self.pointwise(md, rows, rhs, want_flux=want_flux, max_chunk=max_chunk))
        if not res:
            res = self.apply(md, rows, "Cinv", rhs, want_flux=want_flux, max_chunk=max_chunk)
            res["alpha"] = res.pop("out")
        return res

    def diagnose_banded(self, md, params, rhs=None, want=("alpha",), want_flux=False, max_chunk=None, solver="banded"):
        """The residual diagnostics on the band + Woodbury solver (sf_diagnose_banded_batch): what :meth:`apply` with "Cinv",
        :meth:`pointwise` and :meth:`decompose` give from the dense factor, from one keeping sweep per walker.  params, rhs:
        as for :meth:`apply`.  want: some of "alpha" (B, nrhs, n; always returned), "cinv_diag" (B, n), "cov_diag" (B, n),
        "comp" (B, 3 + n_local, nrhs, n).  Returns dict of numpy arrays: those, info and, asked for, flux (B, n); NaN rows
        where info != 0.  Values agree with the dense calls to rounding, not bit for bit.

        The walkers whose host half-width bound fits the LDS window go in one group at the group's largest bound (so that
        chunks and sub-batches of it give the same bits).  More right-hand sides than the window takes at that half-width
        (:meth:`diagnose_banded_max_nrhs`) are cut into groups of that size (:func:`rhs_groups`), one call each; the two
        diagonals are taken from the first.  solver: "banded" -- the other walkers come back with info = -4 and NaN rows;
        "auto" -- they, and walkers with the internal status -5, go through the dense calls (:func:`finish_structured`)."""
        torch = _torch()
        check_solver(solver, ("banded", "auto"))
        want = diagnose_wants(want)
        rows, hw = self._host_rows_and_bound(md, params)
        B = rows.shape[0]
        with torch.cuda.device(self.dev):
            R, nrhs, per_walker = self._rhs_on_device(rhs, B)
        fits = hw <= self.banded_window_halfwidth()
        out = refused_output(B, self._diagnose_shapes(md, want, nrhs, want_flux))
        del out["lnl"]  # (no likelihood here)
        idx = np.nonzero(fits)[0]
        if idx.size:
            W = int(hw[idx].max())
            with torch.cuda.device(self.dev):
                Rg = R[torch.from_numpy(idx).to(self.dev)] if per_walker else R
            for g, cols in enumerate(rhs_groups(nrhs, self.diagnose_banded_max_nrhs(W))):
                # (the diagonals, the flux and the status do not depend on the right-hand sides: the first group's)
                first = g == 0
                got = self._diagnose_banded_group(md, rows[idx], W, Rg, per_walker, cols,
                                                  want if first else tuple(w for w in want if w in ("alpha", "comp")),
                                                  want_flux and first, max_chunk)
                for key, v in got.items():
                    if key in ("alpha", "comp"):
                        out[key][idx, ..., cols[0]:cols[1], :] = v
                    elif first:
                        out[key][idx] = v
                    elif key == "info":  # (a later group's status counts where the first had none)
                        out[key][idx] = np.where(out[key][idx] == 0, v, out[key][idx])
            bad = out["info"][idx] != 0  # (every row of a failed walker is NaN, whichever group reported it)
            for key in out:
                if key not in ("info", "flux") and bad.any():
                    out[key][idx[bad]] = np.nan

        def dense(rest):
            sub = rhs
            if per_walker:
                sub = R[torch.from_numpy(rest).to(self.dev)]
            return self._diagnose_dense(md, rows[rest], sub, want, want_flux, max_chunk)

        return finish_structured(out, fits, solver, dense)

    def _run_grad(self, name, md, params, lead, slots, workspace_bytes, want_flux, max_chunk):
        """:meth:`_run_chunked` for ``sf_<name>(ctx, &md, B, P, *lead, lnl, grad, grad_stride, flux, info, ws, ...)``: the two
        likelihood-and-gradient calls.  ``lead``: the host arguments in front; ``slots``: the gradient columns wanted (the
        buffer has at least one); ``workspace_bytes(units)``: the call's size query."""
        stride = max(slots, 1)
        with _torch().cuda.device(self.dev):
            P = self._rows(params)
            buffers, download = self._outputs(int(P.shape[0]), {"lnl": (), "grad": (stride,)}, want_flux)

            def args(bufs, lo, hi):
                (lnl, grad), info, flux = bufs
                return (*lead, lnl[lo:hi], grad[lo:hi], stride, flux[lo:hi] if want_flux else None, info[lo:hi])

            def sliced(bufs):
                res = download(bufs)
                res["grad"] = res["grad"][:, :slots]
                return res

            return self._run_chunked(name, md, P, max_chunk, workspace_bytes, buffers, args, sliced)

    def loglike_grad(self, md, params, want_flux=False, max_chunk=None, solver="dense"):
        """The likelihood and its gradient in the covariance hyper-parameters (sf_loglike_grad_batch).  params: (B, stride)
        rows as for :meth:`loglike`.  Returns dict of numpy arrays: lnl (B,) and info (B,) with :meth:`loglike`'s bits, grad
        (B, slots) with the slots in parameter-row order (log_amp, log_ls of the global kernel if the model has one, then mu,
        log_amp, log_sigma per local kernel), NaN rows where info != 0, and, asked for, flux (B, n).  Chunked and retried
        like :meth:`apply`.

        solver: "dense"  -- the dense factor and the support blocks of its inverse (sf_loglike_grad_batch);
                "banded" -- band + rank-m Woodbury solve, the band of Bd^-1 by selected inversion and the contraction over
                            the band (sf_loglike_banded_grad_batch without mean slots): lnl and info as
                            :meth:`loglike_mean_grad` gives them under "banded", grad agrees with the dense call to rounding;
                            walkers whose covariance support exceeds the LDS window come back with info = -4;
                "auto"   -- banded for the walkers whose half-width bound fits the window, dense for the rest."""
        check_solver(solver)
        if solver != "dense":
            return self.loglike_banded_grad(md, params, (), True, want_flux=want_flux, max_chunk=max_chunk, solver=solver)
        return self._run_grad("loglike_grad_batch", md, params, (), R.cov_grad_slots(md),
                              lambda units: self.loglike_grad_workspace_bytes(md, units), want_flux, max_chunk)

    def loglike_banded_grad_workspace_bytes(self, md, B, halfwidth, nslots, want_cov):
        return self._size_query("loglike_banded_grad_", md, B, halfwidth, nslots, int(bool(want_cov)))

    def loglike_banded_grad(self, md, params, slots, want_cov, want_flux=False, max_chunk=None, solver="banded"):
        """The likelihood and its gradient on the band solver in one call (sf_loglike_banded_grad_batch): the mean-flux
        columns ``slots`` as :meth:`loglike_mean_grad` gives them under the same solver (same bits), and behind them, with
        ``want_cov``, the covariance slots of :meth:`loglike_grad`.  solver: "banded" or "auto", as for
        :meth:`loglike_mean_grad`; under "auto" the walkers the window does not take go through the two dense calls."""
        check_solver(solver, ("banded", "auto"))
        slots = [int(v) for v in slots]
        if not slots and not want_cov:
            raise ValueError("nothing to differentiate: no mean slots and want_cov is false")
        return self._banded_grad(md, params, slots, want_cov, want_flux, max_chunk, solver)

    def loglike_mean_grad_workspace_bytes(self, md, B, nslots):
        return self._size_query("loglike_mean_grad_", md, B, nslots)

    def loglike_banded_mean_grad_workspace_bytes(self, md, B, halfwidth, nslots):
        return self._size_query("loglike_banded_mean_grad_", md, B, halfwidth, nslots)

    def loglike_mean_grad(self, md, params, slots, want_flux=False, max_chunk=None, solver="dense"):
        """The likelihood and its gradient in the mean-flux parameters (sf_loglike_mean_grad_batch).  params: (B, stride) rows
        as for :meth:`loglike`; slots: the columns of the parameter row to differentiate in (vsini = 0, vz = 1, log_scale = 2,
        the grid, Chebyshev and Av columns), each at most once, at most MEAN_GRAD_MAX_SLOTS.  Returns dict of
        numpy arrays: lnl (B,) and info (B,) with :meth:`loglike`'s bits, grad (B, len(slots)) in the order of ``slots``, NaN rows
        where info != 0, and, asked for, flux (B, n).  Chunked and retried like :meth:`apply`.

        solver: "dense"  -- the dense factor (sf_loglike_mean_grad_batch);
                "banded" -- band + rank-m Woodbury solve with a backward sweep (sf_loglike_banded_mean_grad_batch): lnl and
                            grad agree with the dense call to rounding, not bit for bit;
                            walkers whose covariance support exceeds the LDS window come back with info = -4;
                "auto"   -- banded for the walkers whose half-width bound fits the window, dense for the rest."""
        check_solver(solver)
        if solver != "dense":
            return self._banded_grad(md, params, slots, False, want_flux, max_chunk, solver)
        slots = [int(v) for v in slots]
        nslots = len(slots)
        h_slots = (C.c_int * max(nslots, 1))(*slots)
        return self._run_grad("loglike_mean_grad_batch", md, params, (h_slots, nslots), nslots,
                              lambda units: self.loglike_mean_grad_workspace_bytes(md, units, nslots), want_flux, max_chunk)

    def _banded_grad(self, md, params, slots, want_cov, want_flux, max_chunk, solver):
        """The mean columns ``slots`` and, with ``want_cov``, the covariance slots behind them on the band solver
        (:meth:`_grad_structured`): a mean-only request is sf_loglike_banded_mean_grad_batch, one with covariance columns
        sf_loglike_banded_grad_batch; the walkers that go to the dense solver go through its two calls."""
        slots = [int(v) for v in slots]
        nslots, want_cov = len(slots), bool(want_cov)
        ncols = nslots + (R.cov_grad_slots(md) if want_cov else 0)
        h_slots = (C.c_int * max(nslots, 1))(*slots)
        call, tail = ("loglike_banded_grad_", (1,)) if want_cov else ("loglike_banded_mean_grad_", ())
        size_query = getattr(self, call + "workspace_bytes")

        def banded(rows, W):
            return self._run_grad(call + "batch", md, rows, (W, h_slots, nslots, *tail), ncols,
                                  lambda units: size_query(md, units, W, nslots, *tail), want_flux, max_chunk)

        def dense(rows):
            parts = []
            if nslots:
                parts.append(self.loglike_mean_grad(md, rows, slots, want_flux=want_flux, max_chunk=max_chunk, solver="dense"))
            if want_cov:
                parts.append(self.loglike_grad(md, rows, want_flux=want_flux, max_chunk=max_chunk, solver="dense"))
            res = dict(parts[0])
            res["grad"] = np.concatenate([q["grad"] for q in parts], axis=1)
            return res

        return self._grad_structured(md, params, ncols, banded, dense, want_flux, solver)

    def _grad_structured(self, md, params, ncols, banded, dense, want_flux, solver):
        """A likelihood-and-gradient call on the band solver: the walkers whose host half-width bound fits the LDS window in
        one group with the group's largest bound (so that chunks of it give the same bits) through ``banded(rows, W)``; the
        rest, and walkers with the internal status, through ``dense(rows)`` under "auto" (the internal status under "banded"
        too: :func:`finish_structured`).  Both return the dict of :meth:`_run_grad` with ``ncols`` gradient columns."""
        rows, hw = self._host_rows_and_bound(md, params)
        fits = hw <= self.banded_window_halfwidth()
        out = refused_output(rows.shape[0], dict(grad=(ncols,), **({"flux": (self.n,)} if want_flux else {})))
        idx = np.nonzero(fits)[0]
        if idx.size:
            got = banded(rows[idx], int(hw[idx].max()))
            if want_flux:  # (the call returns the residual: model minus data)
                got["flux"] = got["flux"] + self._keep[1][None, :]
            for key, v in got.items():
                out[key][idx] = v
        return finish_structured(out, fits, solver, lambda rest: dense(rows[rest]))

    # ------------------------------------------------------------------ Fisher information in the mean-flux parameters
    def fisher_mean_workspace_bytes(self, md, B, nslots):
        return self._size_query("fisher_mean_", md, B, nslots)

    def fisher_banded_mean_workspace_bytes(self, md, B, halfwidth, nslots):
        return self._size_query("fisher_banded_mean_", md, B, halfwidth, nslots)

    def fisher_banded_max_slots(self, halfwidth):
        """Most columns one sf_fisher_banded_mean_batch call takes at this half-width (0: none)."""
        return max(int(self.lib.sf_fisher_banded_max_slots(self.ctx, int(halfwidth))), 0) if self.n else 0

    def _run_fisher(self, name, md, params, lead, nslots, resid, workspace_bytes, max_chunk):
        """:meth:`_run_chunked` for ``sf_<name>(ctx, &md, B, P, *lead, lnl, fisher, nslots^2, [resid,] info, ws, ...)``.
        ``resid``: None -- the call has no such argument (the dense one); False -- NULL; True -- a (B, n) buffer, returned
        under "resid" (model minus data)."""
        with _torch().cuda.device(self.dev):
            P = self._rows(params)
            buffers, download = self._outputs(int(P.shape[0]), {"lnl": (), "fisher": (nslots, nslots)}, bool(resid))

            def args(bufs, lo, hi):
                (lnl, fisher), info, flux = bufs
                tail = () if resid is None else (flux[lo:hi] if resid else None,)
                return (*lead, lnl[lo:hi], fisher[lo:hi], nslots * nslots, *tail, info[lo:hi])

            def named(bufs):
                res = download(bufs)
                if resid:
                    res["resid"] = res.pop("flux")
                return res

            # (a size of 0: the call refuses its arguments and says why -- it gets a workspace that is not NULL to say it)
            return self._run_chunked(name, md, P, max_chunk, lambda units: max(workspace_bytes(units), 256), buffers, args, named)

    def fisher_mean(self, md, params, slots, solver="dense", max_chunk=None):
        """The likelihood and the Fisher information of the mean-flux parameters at fixed covariance, ``F_ij = fdot_i^T C^-1
        fdot_j`` with ``fdot_j = d f / d theta_j`` (sf_fisher_mean_batch).  This is the Gauss-Newton matrix: the term
        ``1/2 tr(C^-1 dC_i C^-1 dC_j)`` of a grid parameter (X sits inside the emulator's covariance) is left out (the
        covariance hyper-parameters' block: :meth:`fisher_cov`).  params, slots: as for :meth:`loglike_mean_grad`.  Returns dict of numpy arrays: lnl (B,), fisher (B, p, p) in the order of ``slots``,
        bit-symmetric, NaN where info != 0, and info (B,).  Chunked and retried like :meth:`loglike_mean_grad`.

        solver: "dense"  -- the dense factor, ``F = Z^T Z`` with ``Z = L^-1 J`` (lnl and info with :meth:`loglike`'s bits);
                "banded" -- ONE sweep of the band + Woodbury solver over the rows [r; Y; J] (sf_fisher_banded_mean_batch), one
                            half-width for every chunk; agrees with the dense call to rounding.  Walkers whose covariance
                            support exceeds the LDS window at this row count come back with info = -4;
                "auto"   -- banded for the walkers whose half-width bound fits that window, dense for the rest and for
                            walkers with the internal status, merged by row."""
        check_solver(solver)
        slots = [int(v) for v in slots]
        nslots = len(slots)
        if not nslots:
            raise ValueError("no column to take the Fisher information in")
        h_slots = (C.c_int * nslots)(*slots)
        if solver == "dense":
            return self._run_fisher("fisher_mean_batch", md, params, (h_slots, nslots), nslots, None,
                                    lambda units: self.fisher_mean_workspace_bytes(md, units, nslots), max_chunk)
        rows, hw = self._host_rows_and_bound(md, params)
        # "banded": every walker the window of the likelihood's 1 + m rows takes, at the group's largest bound -- the library
        # refuses the call (ValueError) if that lies beyond the window at 1 + m + p rows; "auto": only the walkers that fit there
        fits = hw <= self.banded_window_halfwidth()
        if solver == "auto":
            fits = np.array([self.fisher_banded_max_slots(int(v)) >= nslots for v in hw], dtype=bool)
        out = refused_output(rows.shape[0], dict(fisher=(nslots, nslots)))
        idx = np.nonzero(fits)[0]
        if idx.size:
            W = int(hw[idx].max())
            got = self._run_fisher("fisher_banded_mean_batch", md, rows[idx], (W, h_slots, nslots), nslots, False,
                                   lambda units: self.fisher_banded_mean_workspace_bytes(md, units, W, nslots), max_chunk)
            for key, v in got.items():
                out[key][idx] = v
        return finish_structured(out, fits, solver, lambda rest: self.fisher_mean(md, rows[rest], slots, "dense", max_chunk))

    # ------------------------------------------------------------------ Fisher information in the covariance hyper-parameters
    def fisher_cov_workspace_bytes(self, md, B):
        return self._size_query("fisher_cov_", md, B)

    def fisher_cov(self, md, params, max_chunk=None):
        """The likelihood and the Fisher information of the covariance hyper-parameters, ``F_ij = 1/2 tr(C^-1 dC_i C^-1
        dC_j)`` (sf_fisher_cov_batch), in the slots of :meth:`loglike_grad`: log_amp, log_ls of the global kernel if the model has
        one, then mu, log_amp, log_sigma per local kernel.  params: (B, stride) rows as for :meth:`loglike`.  Returns dict of
        numpy arrays: lnl (B,) and info (B,) with :meth:`loglike`'s bits, fisher (B, s, s), bit-symmetric, NaN where info != 0.
        The dense factor only.  Chunked and retried like :meth:`loglike_grad`; a chunked call gives the same bits."""
        s = R.cov_grad_slots(md)
        if not s:
            raise ValueError("nothing to differentiate: the model has no global and no local kernel")
        return self._run_fisher("fisher_cov_batch", md, params, (), s, None, lambda units: self.fisher_cov_workspace_bytes(md, units),
                                max_chunk)

    # ------------------------------------------------------------------ score scan for a new local kernel
    def local_scan_workspace_bytes(self, md, B, ncand):
        return self._size_query("local_scan_", md, B, ncand)

    def local_scan(self, md, params, cand, max_chunk=None):
        """The score scan for a NEW local kernel at amplitude 0 (sf_local_scan_batch): for every walker and every candidate
        ``cand[q] = (mu, sigma in km/s)``, shared by the walkers, ``quad = alpha^T k alpha``, ``trace = tr(C^-1 k)`` and ``fisher =
        1/2 tr(C^-1 k C^-1 k)`` with ``k`` the matrix a local kernel of that centre and width adds at amplitude 1 and ``alpha = C^-1
        r``: ``1/2 (quad - trace)`` is the derivative of lnL in the new amplitude, ``fisher`` its information.  params: (B,
        stride) rows as for :meth:`loglike`; the model may have no structured kernel at all.  Returns dict of numpy arrays: quad,
        trace, fisher (B, ncand) -- zeros for a candidate with no pixel in reach, NaN for one whose patch is wider than
        LOCAL_SCAN_MAX_PATCH pixels and for walkers with info != 0 --, lnl (B,) and info (B,) with :meth:`loglike`'s bits.  The
        dense factor only.  Chunked and retried like :meth:`loglike_grad`; a candidate's numbers are the same bits whatever the
        chunk, the batch and the other candidates are."""
        torch = _torch()
        cand = np.ascontiguousarray(np.asarray(cand, dtype=np.float64))
        if cand.ndim != 2 or cand.shape[1] != 2 or not cand.shape[0]:
            raise ValueError(f"cand of shape {cand.shape}: expected (ncand, 2) rows of mu, sigma with ncand >= 1")
        ncand = int(cand.shape[0])
        with torch.cuda.device(self.dev):
            P = self._rows(params)
            Cd = to_dev(cand, self.dev)
            buffers, download = self._outputs(int(P.shape[0]), {"out": (ncand, 3), "lnl": ()}, False)

            def args(bufs, lo, hi):
                (out, lnl), info, _ = bufs
                return (Cd, ncand, out[lo:hi], lnl[lo:hi], info[lo:hi])

            def named(bufs):
                res = download(bufs)
                out = res.pop("out")
                res.update(quad=out[:, :, 0].copy(), trace=out[:, :, 1].copy(), fisher=out[:, :, 2].copy())
                return res

            # (a size of 0: the call refuses its arguments and says why -- it gets a workspace that is not NULL to say it)
            size = lambda units: max(self.local_scan_workspace_bytes(md, units, ncand), 256)  # noqa: E731
            return self._run_chunked("local_scan_batch", md, P, max_chunk, size, buffers, args, named)

    def loglike_device(self, md, P_dev, out_lnl, info=None):
        """Enqueue-only variant for bench.py: device tensors in/out, no synchronisation."""
        self._call("loglike_batch", md, int(P_dev.shape[0]), P_dev, out_lnl, None, None, None, None, info)

    def forward(self, md, params):
        """SpectrumModel.__call__ for B rows: flux (B, n), cov (B, n, n), log_scale, info."""
        torch = _torch()
        with torch.cuda.device(self.dev):
            P = self._rows(params)
            B = int(P.shape[0])
            flux = empty((B, self.n), self.dev)
            cov = empty((B, self.n, self.n), self.dev)
            lsc = empty((B,), self.dev)
            info = empty((B,), self.dev, torch.int32)
            self._call("forward_batch", md, B, P, flux, cov, lsc, info)
            return dict(
                flux=flux.cpu().numpy(), cov=cov.cpu().numpy(), log_scale=lsc.cpu().numpy(),
                info=info.cpu().numpy(),
            )

    def cov_fill(self, md, params, ld=None, lower_only=False, add_jitter=False, guard=0):
        """The fused covariance fill alone (sf_cov_fill_batch): (B, n, ld) array, row stride ``ld`` >= n (columns
        beyond n are left as allocated: zero here).  Exactly n rows per matrix are written -- no identity padding, that
        belongs to the library's own workspace layout.  ``guard`` > 0 appends that many sentinel doubles (-7.0) behind the
        last matrix and returns them as a third value (tests: nothing may be written past the caller's array)."""
        torch = _torch()
        with torch.cuda.device(self.dev):
            P = self._rows(params)
            B = int(P.shape[0])
            ld = int(ld or self.n)
            buf = torch.zeros((B * self.n * ld + int(guard),), dtype=torch.float64, device=self.dev)
            if guard:
                buf[B * self.n * ld:] = -7.0
            cov = buf[: B * self.n * ld].view(B, self.n, ld)
            info = empty((B,), self.dev, torch.int32)
            self._call("cov_fill_batch", md, B, P, cov, ld, self.n * ld, int(lower_only), int(add_jitter), info)
            if guard:
                return cov.cpu().numpy(), info.cpu().numpy(), buf[B * self.n * ld:].cpu().numpy()
            return cov.cpu().numpy(), info.cpu().numpy()

    def cov_fill_device(self, md, P_dev, cov, ld, stride, lower_only=False, add_jitter=True, info=None):
        """Enqueue-only sf_cov_fill_batch into a caller-held device array (bench.py's fill leg): no host copies."""
        torch = _torch()
        with torch.cuda.device(self.dev):
            self._call("cov_fill_batch", md, int(P_dev.shape[0]), P_dev, cov, int(ld), int(stride), int(lower_only),
                       int(add_jitter), info)

    def transform(self, md, params):
        torch = _torch()
        with torch.cuda.device(self.dev):
            P = self._rows(params)
            B = int(P.shape[0])
            flux = empty((B, self.n), self.dev)
            X = empty((B, self.m, self.n), self.dev)
            resid = empty((B, self.n), self.dev)
            lsc = empty((B,), self.dev)
            info = empty((B,), self.dev, torch.int32)
            self._call("transform_batch", md, B, P, flux, X, resid, lsc, info)
            return dict(
                flux=flux.cpu().numpy(), X=X.cpu().numpy(), resid=resid.cpu().numpy(),
                log_scale=lsc.cpu().numpy(), info=info.cpu().numpy(),
            )

    def _grid_rows(self, grid_params):
        """(B, P) grid points as the C-ABI rows of the emulator queries (descriptor with log_scale only): md, rows."""
        gp = np.atleast_2d(np.asarray(grid_params, dtype=np.float64))
        md = self.model_desc(0, 0, 1, 0, 0, 0)
        rows = np.zeros((gp.shape[0], self.param_stride(md)))
        rows[:, R.NORM] = 1.0
        rows[:, R.RowLayout(self.P, md).grid] = gp
        return md, rows

    def emulator_query(self, grid_params):
        """grid_params: (B, P).  Returns mu (B, m), cov (B, m, m), info (B,)."""
        torch = _torch()
        md, rows = self._grid_rows(grid_params)
        B = rows.shape[0]
        with torch.cuda.device(self.dev):
            P = to_dev(rows, self.dev)
            mu = empty((B, self.m), self.dev)
            cov = empty((B, self.m, self.m), self.dev)
            info = empty((B,), self.dev, torch.int32)
            self._call("emulator_query_batch", md, B, P, mu, cov, info)
            return mu.cpu().numpy(), cov.cpu().numpy(), info.cpu().numpy()

    def emulator_query_joint(self, grid_params):
        """grid_params: (B, P).  Joint conditional over the B points, component-major: mu (B*m,), cov (B*m, B*m)."""
        torch = _torch()
        md, rows = self._grid_rows(grid_params)
        B = rows.shape[0]
        with torch.cuda.device(self.dev):
            P = to_dev(rows, self.dev)
            mu = empty((B * self.m,), self.dev)
            cov = empty((B * self.m, B * self.m), self.dev)
            info = empty((B,), self.dev, torch.int32)
            self._call("emulator_joint_batch", md, B, P, mu, cov, info)
            return mu.cpu().numpy(), cov.cpu().numpy(), info.cpu().numpy()
