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
# the names of the layers below, re-exported: the runtime every call shares and the multi-order plans
from ._runtime import (  # noqa: F401
    INFO_MESSAGES, APPLY_OPS, MEAN_GRAD_MAX_SLOTS, MAX_LOCAL, LOCAL_SCAN_MAX_PATCH, INFO_BANDWIDTH, INFO_INTERNAL,
    HBM_RESERVE, _torch, check_solver, current_stream, device_of, empty, fetch_results, finish_structured,
    grow_workspace, persistent_status, ptr, recover_from_internal, refused_output, result_buffers, retry_internal,
    run_chunked, stream_ptr, to_dev, units_that_fit, workspace)
from ._multi import (  # noqa: F401
    BandedMultiFisherPlan, BandedMultiGradPlan, BandedMultiScanPlan, MultiGradPlan, MultiPlan, _BandedFisherUnits,
    _BandedScanUnits, _BandedUnits, banded_units, collect_multi, column_map_csr, fisher_banded_multi,
    local_scan_banded_multi, loglike_banded_multi_grad, loglike_multi, loglike_multi_grad, merge_units, model_desc_key,
    reduce_fisher_host, reduce_orders_host, rerouted_units, scan_cand_ptr, scan_mean_host, scan_out_offsets, scan_rounds,
    scan_routes)

C_KMS = 2.99792458e5


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


def local_scan_route(solver, patch_pixels, limit):
    """Which solver a scan of candidates with ``patch_pixels`` pixels each goes to when ``solver`` is "banded" or "auto" and the
    band solver serves patches of at most ``limit`` pixels (:meth:`DeviceOrder.local_scan_banded_max_patch`; 0: it does not take
    the order).  "auto" with a candidate beyond the limit, or without one, is "dense" for the whole call; "banded" without a limit
    is a ``ValueError`` (with one, the device marks the candidates beyond it NaN).  Pure host logic."""
    check_solver(solver, ("banded", "auto"))
    wide = bool(np.any(np.asarray(patch_pixels) > limit))
    if solver == "auto":
        return "dense" if limit < 1 or wide else "auto"
    if limit < 1:
        raise ValueError('the band solver does not take this order (no LDS window for its 1 + m rows, or a wavelength grid that is '
                         'not strictly increasing): use solver="dense" or "auto"')
    return "banded"


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

    def local_scan_banded_max_patch(self, md):
        """Widest patch in pixels that :meth:`local_scan` serves on the band solver (sf_local_scan_banded_max_patch): the widest
        half-width of the LDS window for the order's 1 + m rows, plus one; 0: the band solver does not take this order."""
        return max(int(self.lib.sf_local_scan_banded_max_patch(self.ctx, C.byref(md))), 0) if self.n else 0

    def local_scan_banded_workspace_bytes(self, md, B, ncand):
        return self._size_query("local_scan_banded_", md, B, ncand)

    def _local_scan_call(self, name, md, params, cand, max_chunk, workspace_bytes):
        """:meth:`_run_chunked` for ``sf_<name>(ctx, &md, B, P, cand, ncand, out, lnl, info, ws, ...)``: the two scans."""
        torch = _torch()
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
            size = lambda units: max(workspace_bytes(md, units, ncand), 256)  # noqa: E731
            return self._run_chunked(name, md, P, max_chunk, size, buffers, args, named)

    def local_scan(self, md, params, cand, max_chunk=None, solver="dense"):
        """The score scan for a NEW local kernel at amplitude 0 (sf_local_scan_batch): for every walker and every candidate
        ``cand[q] = (mu, sigma in km/s)``, shared by the walkers, ``quad = alpha^T k alpha``, ``trace = tr(C^-1 k)`` and ``fisher =
        1/2 tr(C^-1 k C^-1 k)`` with ``k`` the matrix a local kernel of that centre and width adds at amplitude 1 and ``alpha = C^-1
        r``: ``1/2 (quad - trace)`` is the derivative of lnL in the new amplitude, ``fisher`` its information.  params: (B,
        stride) rows as for :meth:`loglike`; the model may have no structured kernel at all.  Returns dict of numpy arrays: quad,
        trace, fisher (B, ncand) -- zeros for a candidate with no pixel in reach, NaN for one whose patch is wider than
        LOCAL_SCAN_MAX_PATCH pixels and for walkers with info != 0 --, lnl (B,) and info (B,) with :meth:`loglike`'s bits.
        Chunked and retried like :meth:`loglike_grad`; a candidate's numbers are the same bits whatever the chunk, the batch and
        the other candidates are.

        solver: "dense"  -- the dense factor and the tiles of its inverse (sf_local_scan_batch);
                "banded" -- band + rank-m Woodbury solve and the selected inversion at the LDS window's widest half-width, whatever
                            the walkers' own support (sf_local_scan_banded_batch): all walkers in one group, values agree with the
                            dense call to rounding; a candidate whose patch is wider than :meth:`local_scan_banded_max_patch`
                            pixels is NaN for every walker; walkers whose covariance support exceeds that half-width come back
                            with info = -4, lnl = -inf and NaN rows;
                "auto"   -- if a candidate's patch (:func:`local_scan_patches`) is wider than the banded limit, or the band solver
                            does not take the order, the whole call is the dense one (one factorisation serves every candidate:
                            splitting the list would pay for both); otherwise banded, with the walkers that do not fit, and those
                            with the internal status -5, through the dense call (:func:`finish_structured`)."""
        check_solver(solver)
        cand = np.ascontiguousarray(np.asarray(cand, dtype=np.float64))
        if cand.ndim != 2 or cand.shape[1] != 2 or not cand.shape[0]:
            raise ValueError(f"cand of shape {cand.shape}: expected (ncand, 2) rows of mu, sigma with ncand >= 1")
        if solver != "dense":
            limit = self.local_scan_banded_max_patch(md)
            lo, hi = local_scan_patches(self._keep[0], cand)
            solver = local_scan_route(solver, hi - lo + 1, limit)
        if solver == "dense":
            return self._local_scan_call("local_scan_batch", md, params, cand, max_chunk, self.local_scan_workspace_bytes)
        rows, hw = self._host_rows_and_bound(md, params)
        fits = hw <= limit - 1
        out = refused_output(rows.shape[0], {key: (cand.shape[0],) for key in ("quad", "trace", "fisher")})
        idx = np.nonzero(fits)[0]
        if idx.size:
            got = self._local_scan_call("local_scan_banded_batch", md, rows[idx], cand, max_chunk,
                                        self.local_scan_banded_workspace_bytes)
            for key, v in got.items():
                out[key][idx] = v
        return finish_structured(out, fits, solver, lambda rest: self.local_scan(md, rows[rest], cand, max_chunk))

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
