"""
Multi-order calls: the (order x walker) units of several orders of ONE device in one launch sequence (csrc/sf_multi.cpp,
csrc/sf_multi_banded.cpp).  One frame for a unit list (:class:`MultiPlan`: checks, upload, workspace, the cut into calls), four
kinds of call on it -- likelihood, gradient, gradient and Fisher information on the band solver -- and one dispatcher for the
band solver's two; the score scan for new local kernels on the band solver is a fifth kind with a dispatcher of its own.  The orders are :class:`starfish_amd._device.DeviceOrder` objects; only their methods are called.
"""

import collections
import ctypes as C

import numpy as np

from . import _lib
from . import _rows as R
from ._runtime import (INFO_INTERNAL, INFO_BANDWIDTH, MEAN_GRAD_MAX_SLOTS, _torch, check_solver, empty, fetch_results,
                       grow_workspace, ptr, refused_output, result_buffers, retry_internal, stream_ptr, to_dev, units_that_fit)


def model_desc_key(md):
    """The fields of a ModelDesc as a hashable tuple (two orders may share a multi-order call only if equal)."""
    return tuple(int(getattr(md, name)) for name, _ in md._fields_)


def cut_units(sizes, cap):
    """The units of orders with ``sizes[i]`` units each, in unit order, cut into pieces of at most ``cap`` units: a list of
    pieces, each a list of ``(order, lo, hi)`` -- the units lo .. hi of that order.  Pure host logic."""
    pieces, cur, cur_n = [], [], 0
    for i, n in enumerate(sizes):
        lo = 0
        while lo < n:
            take = min(n - lo, cap - cur_n)
            cur.append((i, lo, lo + take))
            cur_n += take
            lo += take
            if cur_n == cap:
                pieces.append(cur)
                cur, cur_n = [], 0
    if cur:
        pieces.append(cur)
    return pieces


def split_units(host, sizes, widths=None):
    """Per order a dict of its units' rows of the (units, ...) arrays ``host[key]``; ``widths``: key -> per order, how much of
    every trailing dimension is the order's own."""
    ends = np.cumsum(sizes)
    out = [{key: v[hi - n:hi] for key, v in host.items()} for n, hi in zip(sizes, ends)]
    for key, ks in (widths or {}).items():
        for o, k in zip(out, ks):
            o[key] = np.ascontiguousarray(o[key][(slice(None),) + (slice(0, k),) * (o[key].ndim - 1)])
    return out


def collect_multi(quad, info, sizes):
    return split_units(fetch_results(quad, info), sizes)


def normalise_requests(orders, mds, requests):
    """``requests[i] = (mean_columns, want_cov)`` of a gradient plan as lists of int and bool, and the slots of every order."""
    if len(requests) != len(orders):
        raise ValueError(f"multi-order gradient: {len(requests)} requests for {len(orders)} orders")
    requests = [([int(c) for c in cols], bool(cov)) for cols, cov in requests]
    slots = [len(cols) + (R.cov_grad_slots(md) if cov else 0) for (cols, cov), md in zip(requests, mds)]
    if not any(slots):
        raise ValueError("multi-order gradient: nothing to differentiate (no order requests a slot)")
    return requests, slots


def same_walkers(call, sizes):
    """The walkers W of every order, for the order sum ``call``."""
    if len(set(sizes)) != 1:
        raise ValueError(f"{call}: the orders have {sorted(set(sizes))} walkers")
    return sizes[0]


class Call(collections.namedtuple("Call", "segs nseg u0 n models")):
    """One C call of a plan: its segments, the first of its ``n`` units (the pieces of one call are contiguous in unit order)
    and its descriptors; ``orders``: the order index of every segment."""

    def __new__(cls, segs, nseg, u0, n, models, orders):
        self = super().__new__(cls, segs, nseg, u0, n, models)
        self.orders = list(orders)
        return self


class MultiPlan:
    """Device-resident state of a repeated multi-order evaluation (sf_loglike_multi_batch): parameter rows,
    outputs and workspace are allocated once; :meth:`enqueue` only launches.  ``orders`` are
    :class:`DeviceOrder` objects of ONE device, ``rows_list[i]`` the (B_i, stride) C-ABI rows of order i.
    ``md`` is one ModelDesc for every order (all rows of one layout), or a list with one ModelDesc per order
    (sf_loglike_multi_batch_md: orders with their own row layouts still share one batched Cholesky).
    Unit lists that do not fit the free HBM (or ``max_units``) are cut into several calls.

    This class is the frame of every kind of multi-order call and the likelihood kind itself.  The other kinds state their entry
    point and workspace query with the arguments these take beside the frame's, their extra result buffer, the keys of their
    per-order dicts and whether :meth:`collect` retries; they are built by :meth:`_init_requests`.  Every call record
    (``self.calls``, :class:`Call`) carries the order indices of its piece (``self.pieces``, :func:`cut_units`)."""

    entry = "sf_loglike_multi_batch"  # the call :meth:`collect`'s retry names
    retries = True  # collect() runs the batch once more after SF_INFO_INTERNAL (False: the status is left to the dispatcher)
    requests = slots = None  # (the likelihood differentiates nothing)
    halfwidth = None  # the band solver's kinds: the half-width every segment is given

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
                probe = Call(C.byref(one), 1, 0, 1, self._models([i]), [i])
                w1 = self._workspace_bytes(probe)
                one.B = 2
                w2 = self._workspace_bytes(probe)
                pu = max(w2 - w1, 1)
                per_unit, fixed = max(per_unit, pu), max(fixed, w1 - pu)
            lead = orders[0]
            held = lead._ws_multi.numel() if lead._ws_multi is not None else 0
            self.pieces = cut_units(self.sizes, units_that_fit(self.dev, fixed, per_unit, held, max_units or None))
            offs = np.concatenate([[0], np.cumsum(self.sizes)])
            self.calls, need = [], 0
            for piece in self.pieces:
                segs = (_lib.Segment * len(piece))()
                for k, (i, lo, hi) in enumerate(piece):
                    segs[k] = _lib.Segment(orders[i].ctx, ptr(self.P[i][lo:hi]).value, hi - lo, 0)
                idxs = [i for i, _, _ in piece]
                call = Call(segs, len(piece), int(offs[piece[0][0]] + piece[0][1]), sum(hi - lo for _, lo, hi in piece),
                            self._models(idxs), idxs)
                nb = self._workspace_bytes(call)
                if nb == 0:
                    _lib.check(-1, "sf_multi_workspace_bytes")
                need = max(need, nb)
                self.calls.append(call)
            self.ws = grow_workspace(vars(lead), "_ws_multi", need, self.dev)

    def _init_requests(self, orders, mds, rows_list, requests, max_units, halfwidth=None):
        """The constructor of the kinds that differentiate: ``requests`` as :class:`MultiGradPlan` takes them."""
        self.halfwidth = halfwidth if halfwidth is None else int(halfwidth)
        self.requests, self.slots = normalise_requests(orders, mds, requests)
        self.stride = max(self.slots)
        self._slot_arrays = [(C.c_int32 * max(len(cols), 1))(*cols) for cols, _ in self.requests]
        MultiPlan.__init__(self, orders, list(mds), rows_list, max_units=max_units)
        with _torch().cuda.device(self.dev):
            setattr(self, self.extra, self._extra_buffer())

    @staticmethod
    def _desc_array(mds):
        """``const sf_model_desc* const*`` of the given descriptors (the array keeps them alive)."""
        arr = (C.POINTER(_lib.ModelDesc) * len(mds))(*[C.pointer(m) for m in mds])
        arr._keep = mds
        return arr

    def _models(self, idxs):
        """The descriptor argument of a call on these orders."""
        return self._desc_array([self.md[i] for i in idxs]) if self.per_order else C.byref(self.md)

    def _requests_array(self, idxs):
        """``const sf_grad_request*`` of the given orders (the array keeps the column lists alive)."""
        arr = (_lib.GradRequest * len(idxs))()
        for k, i in enumerate(idxs):
            cols, cov = self.requests[i]
            arr[k] = _lib.GradRequest(self._slot_arrays[i], len(cols), int(cov))
        arr._keep = self._slot_arrays
        return arr

    def _plain(self, call):
        """A call in which no order requests a slot is a plain likelihood call."""
        return self.requests is None or not any(self.slots[i] for i in call.orders)

    def _workspace_bytes(self, call):
        if self._plain(call):
            fn = self.lib.sf_multi_workspace_bytes_md if self.per_order else self.lib.sf_multi_workspace_bytes
            return fn(call.segs, call.nseg, call.models)
        return getattr(self.lib, self.query)(call.segs, call.nseg, call.models, self._requests_array(call.orders),
                                             *self._halfwidths(call.nseg), *self._query_strides())

    def _halfwidths(self, nseg):
        """The half-width argument of the band solver's entry points (none of the others')."""
        return () if self.halfwidth is None else ((C.c_int * nseg)(*([self.halfwidth] * nseg)),)

    @property
    def units(self):
        return sum(self.sizes)

    def enqueue(self):
        """Launch only: results land in ``self.quad`` (rows lnl, logdet, sqmah, log_scale; a kind that differentiates leaves
        rows 1 and 2 alone), ``self.info`` and the kind's extra buffer once the device's current stream is done."""
        torch = _torch()
        with torch.cuda.device(self.dev):
            s = stream_ptr(self.dev)
            for call in self.calls:
                out = [ptr(row[call.u0:call.u0 + call.n]) for row in (*self.quad, self.info)]
                lnl, logdet, sqmah, log_scale, info = out
                if self._plain(call):
                    name = "sf_loglike_multi_batch_md" if self.per_order else "sf_loglike_multi_batch"
                    if self.requests is not None:
                        logdet = sqmah = None
                    rc = getattr(self.lib, name)(call.segs, call.nseg, call.models, lnl, logdet, sqmah, log_scale, info, ptr(self.ws),
                                                 self.ws.numel(), s)
                else:
                    name = self.entry
                    rc = getattr(self.lib, name)(call.segs, call.nseg, call.models, self._requests_array(call.orders),
                                                 *self._halfwidths(call.nseg), lnl, log_scale, info,
                                                 ptr(getattr(self, self.extra)[call.u0:call.u0 + call.n]), *self._strides(),
                                                 ptr(self.ws), self.ws.numel(), s)
                _lib.check(rc, name)

    def _per_order(self):
        if self.requests is None:
            return collect_multi(self.quad, self.info, self.sizes)
        rows = dict(lnl=0, log_scale=3)
        host = {key: (self.quad[rows[key]] if key in rows else getattr(self, key)).cpu().numpy() for key in self.keys}
        return split_units(host, self.sizes, {self.extra: self.slots})

    def collect(self):
        """Per order a dict of numpy arrays: lnl, logdet, sqmah, log_scale, info (B,) -- of a kind that differentiates, its
        ``keys`` with the order's own slots of the extra buffer, NaN where info != 0.  Where the kind retries, the whole batch is
        run once more after SF_INFO_INTERNAL (:func:`retry_internal`)."""
        if not self.retries:
            return self._per_order()

        def fetch(again):  # (the first run was enqueued by the caller)
            if again:
                self.enqueue()
            out = self._per_order()
            return out, np.concatenate([o["info"] for o in out])

        return retry_internal(self.lib, self.entry, fetch)

    def reduce(self, sources):
        """The sum over the orders on the device (sf_multi_grad_reduce, sf_multi_fisher_reduce), of what a finished call of a
        kind that differentiates left in the plan's buffers: ``sources[j]`` lists the ``(order, slot)`` pairs whose unit slots
        column j adds, ascending in the order.  Every order must have the same number of walkers W.  Returns numpy ``lnl (W,)``,
        ``grad (W, len(sources))`` or ``fisher (W, len(sources), len(sources))``, ``info (W,)``."""
        torch = _torch()
        name = f"sf_multi_{self.extra}_reduce"
        W, ncols = same_walkers(name, self.sizes), len(sources)
        shape = (ncols,) * (getattr(self, self.extra).ndim - 1)  # a walker's sum: a gradient row or a matrix
        size = int(np.prod(shape))
        width = max(size, 1)
        col_ptr, col_src = column_map_csr(sources)
        with torch.cuda.device(self.dev):
            d_ptr, d_src = torch.from_numpy(col_ptr).to(self.dev), torch.from_numpy(col_src).to(self.dev)
            lnl, total = empty((W,), self.dev), empty((W, width), self.dev)
            info = empty((W,), self.dev, torch.int32)
            rc = getattr(self.lib, name)(len(self.sizes), W, ptr(self.quad[0]), ptr(self.info), ptr(getattr(self, self.extra)),
                                         *self._strides(), ptr(d_ptr), ptr(d_src), ncols, ptr(lnl), ptr(total), width, ptr(info),
                                         stream_ptr(self.dev))
            _lib.check(rc, name)
            return lnl.cpu().numpy(), total.cpu().numpy()[:, :size].reshape((W,) + shape), info.cpu().numpy()


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
    ``max_units``) are cut into several calls, a piece in which no order requests anything is a plain likelihood call.
    :meth:`collect`: per order lnl (B,), grad (B, slots of the order), log_scale (B,), info (B,)."""

    entry, query = "sf_loglike_multi_grad_batch_md", "sf_multi_grad_workspace_bytes_md"
    extra, keys = "grad", ("lnl", "grad", "log_scale", "info")

    def __init__(self, orders, mds, rows_list, requests, max_units=None):
        self._init_requests(orders, mds, rows_list, requests, max_units)

    def _extra_buffer(self):
        return _torch().zeros((self.units, self.stride), dtype=_torch().float64, device=self.dev)

    def _strides(self):
        """What the entry point and the order sum take behind the extra buffer."""
        return (self.stride,)

    _query_strides = _strides  # ... and the workspace query behind the requests


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


class _BandedUnits(MultiPlan):
    """The device side of :class:`BandedMultiGradPlan`: the units the band kernels take, every segment with the half-width
    ``halfwidth`` (sf_loglike_banded_multi_grad_batch_md).  A piece of a cut unit list in which no order requests anything is
    the plain (dense) multi-order likelihood, as in :class:`MultiGradPlan`.  :meth:`collect` does not retry: the band sweep's
    internal status is recomputed densely per unit (:func:`rerouted_units`), not by a second run of the batch."""

    entry, query = "sf_loglike_banded_multi_grad_batch_md", "sf_banded_multi_grad_workspace_bytes_md"
    extra, keys, retries = "grad", MultiGradPlan.keys, False
    _extra_buffer, _strides, _query_strides = MultiGradPlan._extra_buffer, MultiGradPlan._strides, MultiGradPlan._strides

    def __init__(self, orders, mds, rows_list, requests, halfwidth, max_units=None):
        self._init_requests(orders, mds, rows_list, requests, max_units, halfwidth)


class _BandedFisherUnits(MultiPlan):
    """The device side of :class:`BandedMultiFisherPlan`: the units the band kernels take, every segment with the half-width
    ``halfwidth`` (sf_fisher_banded_multi_batch_md).  ``self.fisher``: (units, pmax, pmax), a unit's matrix in its leading
    p_i x p_i block.  :meth:`collect`: per order lnl (B,), fisher (B, p_i, p_i), info (B,); no retry, as :class:`_BandedUnits`."""

    entry, query = "sf_fisher_banded_multi_batch_md", "sf_fisher_banded_multi_workspace_bytes_md"
    extra, keys, retries = "fisher", ("lnl", "fisher", "info"), False
    __init__ = _BandedUnits.__init__

    def _extra_buffer(self):
        return empty((self.units, self.stride, self.stride), self.dev)

    def _strides(self):
        return self.stride, self.stride * self.stride  # (fisher_ld, fisher_stride)

    def _query_strides(self):
        return ()


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
        torch = _torch()
        self.orders, self.mds, self.solver, self.max_units = list(orders), list(mds), solver, max_units
        self.requests, self.slots = normalise_requests(self.orders, self.mds, requests)
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
        """Per order a dict of numpy arrays with the keys of the device side's :meth:`MultiPlan.collect` (lnl (B,), grad (B,
        slots of the order), log_scale (B,), info (B,)); refused units have ``-inf``, NaN and INFO_BANDWIDTH."""
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
        """The sum over the orders of a collected call, as :meth:`MultiPlan.reduce`: on the device (sf_multi_grad_reduce,
        sf_multi_fisher_reduce) when every unit ran on the band kernels and none was re-routed, else by
        :func:`reduce_orders_host` / :func:`reduce_fisher_host` of the collected units -- the same rule, the same bits."""
        kind = self._units.extra
        if self._out is None:
            raise RuntimeError(f"{type(self).__name__}.reduce: collect() first")
        same_walkers(f"sf_multi_{kind}_reduce", self.sizes)
        if self.complete and not self.rerouted:
            return self.plan.reduce(sources)
        host = reduce_fisher_host if kind == "fisher" else reduce_orders_host
        return host(np.stack([o["lnl"] for o in self._out]), np.stack([o["info"] for o in self._out]),
                    [o[kind] for o in self._out], sources)


def loglike_banded_multi_grad(orders, mds, rows_list, requests, solver="banded", max_units=None, sync=True):
    """:func:`loglike_multi_grad` on the band solver (:class:`BandedMultiGradPlan`; ``solver``: "banded" or "auto")."""
    plan = BandedMultiGradPlan(orders, mds, rows_list, requests, solver=solver, max_units=max_units)
    plan.enqueue()
    return plan.collect() if sync else plan


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


def fisher_banded_multi(orders, mds, rows_list, columns, solver="banded", max_units=None, sync=True):
    """The likelihood and the Fisher information of the mean-flux parameters for the (order x walker) units of several orders of
    ONE device on the band solver (:class:`BandedMultiFisherPlan`; ``solver``: "banded" or "auto").  Returns its per-order
    dicts; with ``sync=False`` the un-synchronised plan."""
    plan = BandedMultiFisherPlan(orders, mds, rows_list, columns, solver=solver, max_units=max_units)
    plan.enqueue()
    return plan.collect() if sync else plan


# ------------------------------------------------------------------ score scan for new local kernels, all orders in one pass
SCAN_MAX_CAND = 65535  # candidates per segment and call (sf_local_scan_banded_multi_batch_md)


def scan_rounds(counts, step=SCAN_MAX_CAND):
    """Candidate lists of ``counts[i]`` candidates cut into calls of at most ``step`` per order: a list of rounds, each a list of
    ``(lo, hi, real)`` per order.  Every order stays in every round, so that all calls share one frame: an order whose list is
    used up scans its last candidate once more (``real`` false: the result is dropped).  Pure host logic."""
    counts = [int(c) for c in counts]
    if not counts or min(counts) < 1:
        raise ValueError("the scan needs at least one candidate per order")
    rounds = []
    for r in range(max(-(-c // step) for c in counts)):
        rounds.append([(r * step, min((r + 1) * step, c), True) if r * step < c else (c - 1, c, False) for c in counts])
    return rounds


def scan_cand_ptr(counts):
    """``h_cand_ptr`` of sf_local_scan_banded_multi_batch_md for segments of ``counts[i]`` candidates: (nseg + 1,) int32."""
    return np.concatenate([[0], np.cumsum(np.asarray(counts, dtype=np.int64))]).astype(np.int32)


def scan_out_offsets(sizes, counts):
    """Where the triples of every segment of sf_local_scan_banded_multi_batch_md start, in doubles: ``3 sum_{j<i} B_j ncand_j``,
    (nseg + 1,) int64 -- the last entry is the length of ``d_out``."""
    per = 3 * np.asarray(sizes, dtype=np.int64) * np.asarray(counts, dtype=np.int64)
    return np.concatenate([[0], np.cumsum(per)]).astype(np.int64)


def scan_routes(solver, patch_pixels, limits):
    """Where the scan of every order of a multi-order call goes: ``patch_pixels[i]`` the patch sizes of order i's candidates,
    ``limits[i]`` the widest patch the band solver serves for it (:func:`starfish_amd._device.local_scan_route` per order).
    "banded": every order "banded" -- a candidate beyond the limit, or an order the band solver does not take, is a ``ValueError``
    naming the order; "auto": "auto" per order, "dense" for an order with a candidate beyond the limit or without a limit (its
    units all go through the order's dense scan).  Pure host logic."""
    from ._device import local_scan_route

    routes = []
    for i, (px, limit) in enumerate(zip(patch_pixels, limits)):
        px = np.asarray(px)
        try:
            route = local_scan_route(solver, px, int(limit))
        except ValueError as e:
            raise ValueError(f"order {i}: {e}") from None
        if route == "banded" and px.size and int(px.max()) > int(limit):
            raise ValueError(f"order {i}: a candidate reaches {int(px.max())} pixels: the band solver scans patches of at most "
                             f"{int(limit)} pixels (solver=\"auto\" takes the dense factor for such an order)")
        routes.append(route)
    return routes


def scan_mean_host(quad, trace, fisher, info):
    """sf_local_scan_mean's rule on the host: ``quad``, ``trace``, ``fisher`` (B, ncand), ``info`` (B,).  Per candidate ``z = U /
    sqrt(fisher)`` and ``amp = U / fisher`` with ``U = (quad - trace) / 2`` (NaN where ``fisher == 0``), added over the walkers with
    ``info == 0`` in ascending order, ``s = v_0; s = s + v_1; ...``, and divided by their number: ``(z_mean, amp_mean, count)``;
    no walker: NaN means and 0.  The same operations in the same order as the device: the same bits."""
    quad, trace, fisher = (np.asarray(v, dtype=np.float64) for v in (quad, trace, fisher))
    good = np.nonzero(np.asarray(info) == 0)[0]
    ncand = quad.shape[1]
    if not good.size:
        return np.full(ncand, np.nan), np.full(ncand, np.nan), 0
    score = 0.5 * (quad[good] - trace[good])
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(fisher[good] == 0, np.nan, score / np.sqrt(fisher[good]))
        amp = np.where(fisher[good] == 0, np.nan, score / fisher[good])
    sz, sa = z[0].copy(), amp[0].copy()
    for b in range(1, good.size):
        sz, sa = sz + z[b], sa + amp[b]
    return sz / good.size, sa / good.size, int(good.size)


class _BandedScanUnits(MultiPlan):
    """The device side of :class:`BandedMultiScanPlan`: the units the band kernels take, every order with its own candidates
    ``cands[i]`` (n_i, 2) (sf_local_scan_banded_multi_batch_md).  Candidate lists longer than SCAN_MAX_CAND are scanned in several
    rounds of calls with the same segments, so the same frame (:func:`scan_rounds`).  ``self.out[r]``: the triples of round r,
    unit-major, segment after segment (:func:`scan_out_offsets`).  :meth:`collect`: per order lnl (B,), quad, trace, fisher (B,
    n_i), info (B,); no retry, as :class:`_BandedUnits`."""

    entry, query = "sf_local_scan_banded_multi_batch_md", "sf_local_scan_banded_multi_workspace_bytes_md"
    keys, retries = ("lnl", "quad", "trace", "fisher", "info"), False

    def __init__(self, orders, mds, rows_list, cands, max_units=None):
        self.cands = [np.ascontiguousarray(np.asarray(c, dtype=np.float64)).reshape(-1, 2) for c in cands]
        if len(self.cands) != len(orders):
            raise ValueError(f"multi-order scan: {len(self.cands)} candidate lists for {len(orders)} orders")
        self.rounds = scan_rounds([len(c) for c in self.cands])
        self.counts = [[hi - lo for lo, hi, _ in rnd] for rnd in self.rounds]
        self.cand_ptr = [scan_cand_ptr(c) for c in self.counts]
        MultiPlan.__init__(self, orders, list(mds), rows_list, max_units=max_units)
        self.offsets = [scan_out_offsets(self.sizes, c) for c in self.counts]
        with _torch().cuda.device(self.dev):
            self.d_cand = [to_dev(np.concatenate([c[lo:hi] for c, (lo, hi, _) in zip(self.cands, rnd)]), self.dev)
                           for rnd in self.rounds]
            self.out = [empty((int(off[-1]),), self.dev) for off in self.offsets]

    def _cand_ptr(self, r, idxs):
        """``h_cand_ptr`` of a call on the (consecutive) orders ``idxs`` in round r, into the round's candidate array."""
        p = self.cand_ptr[r]
        return (C.c_int * (len(idxs) + 1))(*[int(p[i]) for i in idxs], int(p[idxs[-1] + 1]))

    def _workspace_bytes(self, call):
        sizes = [self.lib.sf_local_scan_banded_multi_workspace_bytes_md(call.segs, call.nseg, call.models, self._cand_ptr(r, call.orders))
                 for r in range(len(self.rounds))]
        return 0 if min(sizes) == 0 else max(sizes)

    def enqueue(self):
        """Launch only: the triples land in ``self.out``, lnl and log_scale in ``self.quad`` (rows 0 and 3), the status in
        ``self.info`` once the device's current stream is done."""
        with _torch().cuda.device(self.dev):
            s = stream_ptr(self.dev)
            for r in range(len(self.rounds)):
                for call, piece in zip(self.calls, self.pieces):
                    i0, lo0, _ = piece[0]
                    start = int(self.offsets[r][i0]) + 3 * lo0 * self.counts[r][i0]
                    lnl, log_scale, info = (ptr(row[call.u0:call.u0 + call.n]) for row in (self.quad[0], self.quad[3], self.info))
                    rc = self.lib.sf_local_scan_banded_multi_batch_md(call.segs, call.nseg, call.models, ptr(self.d_cand[r]),
                                                                      self._cand_ptr(r, call.orders), ptr(self.out[r][start:]), lnl,
                                                                      log_scale, info, ptr(self.ws), self.ws.numel(), s)
                    _lib.check(rc, self.entry)

    def _triples(self, i):
        """Order i's triples on the device, one (B_i, n, 3) view per round that scans candidates of its own."""
        return [self.out[r][int(self.offsets[r][i]):int(self.offsets[r][i + 1])].view(self.sizes[i], self.counts[r][i], 3)
                for r, rnd in enumerate(self.rounds) if rnd[i][2]]

    def _per_order(self):
        lnl, info = self.quad[0].cpu().numpy(), self.info.cpu().numpy()
        ends = np.cumsum(self.sizes)
        outs = []
        for i, (n, hi) in enumerate(zip(self.sizes, ends)):
            t = np.concatenate([v.cpu().numpy() for v in self._triples(i)], axis=1)
            outs.append(dict(lnl=lnl[hi - n:hi].copy(), quad=t[:, :, 0].copy(), trace=t[:, :, 1].copy(), fisher=t[:, :, 2].copy(),
                             info=info[hi - n:hi].copy()))
        return outs

    def mean(self, i):
        """``(z_mean, amp_mean, count)`` of order i over its walkers with info == 0, on the device (sf_local_scan_mean): only the
        means come to the host."""
        torch = _torch()
        u0 = int(sum(self.sizes[:i]))
        with torch.cuda.device(self.dev):
            info = self.info[u0:u0 + self.sizes[i]]
            count = empty((1,), self.dev, torch.int32)
            means = []
            for t in self._triples(i):
                m = empty((int(t.shape[1]), 2), self.dev)
                rc = self.lib.sf_local_scan_mean(self.sizes[i], int(t.shape[1]), ptr(t), ptr(info), ptr(m), ptr(count), stream_ptr(self.dev))
                _lib.check(rc, "sf_local_scan_mean")
                means.append(m)
            host = np.concatenate([m.cpu().numpy() for m in means], axis=0)
            return host[:, 0].copy(), host[:, 1].copy(), int(count.cpu().numpy()[0])


class BandedMultiScanPlan:
    """The score scan for a new local kernel (:meth:`DeviceOrder.local_scan`) for every (order x walker) unit of ONE device on the
    band + Woodbury solver, all units in one launch sequence (sf_local_scan_banded_multi_batch_md).  ``orders``, ``mds``,
    ``rows_list`` as for :class:`BandedMultiGradPlan`; ``cands[i]``: order i's own candidates, (n_i, 2) rows of mu, sigma in km/s.
    The frame's half-width is the LDS window's widest for 1 + m rows whatever the units' support is, so a unit's bits do not depend
    on the other units or on how the unit list is cut.  Routing by :func:`scan_routes`, :func:`banded_units`,
    :func:`rerouted_units` and :func:`merge_units`: solver "banded" -- a candidate whose patch is wider than the band solver's
    limit is a ``ValueError`` naming the order before any device call, a unit whose covariance support exceeds the window is
    refused (INFO_BANDWIDTH, ``-inf``, NaN rows); "auto" -- such units, the units the kernels flag -4 and every unit of an order
    with a candidate beyond the limit go through the order's dense ``local_scan``.  Status -5 is recomputed densely under either.
    :meth:`collect`: per order the dict :meth:`DeviceOrder.local_scan` returns (quad, trace, fisher (B, n_i), lnl, info);
    :meth:`mean`: per order ``(z_mean, amp_mean, count)``."""

    def __init__(self, orders, mds, rows_list, cands, solver="banded", max_units=None):
        from ._device import local_scan_patches

        check_solver(solver, ("banded", "auto"))
        torch = _torch()
        self.orders, self.mds, self.solver, self.max_units = list(orders), list(mds), solver, max_units
        self.cands = [np.ascontiguousarray(np.asarray(c, dtype=np.float64)) for c in cands]
        if len(self.cands) != len(self.orders):
            raise ValueError(f"multi-order scan: {len(self.cands)} candidate lists for {len(self.orders)} orders")
        for i, c in enumerate(self.cands):
            if c.ndim != 2 or c.shape[1] != 2 or not c.shape[0]:
                raise ValueError(f"order {i}: cand of shape {c.shape}: expected (ncand, 2) rows of mu, sigma with ncand >= 1")
        self.rows = [np.atleast_2d(r.cpu().numpy() if torch.is_tensor(r) else np.asarray(r, dtype=np.float64)) for r in rows_list]
        self.sizes = [int(r.shape[0]) for r in self.rows]
        self.limits = [o.local_scan_banded_max_patch(md) for o, md in zip(self.orders, self.mds)]
        patches = [local_scan_patches(o._keep[0], c) for o, c in zip(self.orders, self.cands)]
        self.routes = scan_routes(solver, [hi - lo + 1 for lo, hi in patches], self.limits)
        self.bounds = [o.halfwidth_bound(md, r) for o, md, r in zip(self.orders, self.mds, self.rows)]
        self.fits = banded_units(self.bounds, [lim - 1 if route != "dense" else -1 for lim, route in zip(self.limits, self.routes)])
        self.idx = [np.nonzero(f)[0] for f in self.fits]
        self.on_device = [i for i, idx in enumerate(self.idx) if idx.size]
        self.plan = None
        if self.on_device:
            self.plan = _BandedScanUnits([self.orders[i] for i in self.on_device], [self.mds[i] for i in self.on_device],
                                         [self.rows[i][self.idx[i]] for i in self.on_device],
                                         [self.cands[i] for i in self.on_device], max_units=max_units)
        self.rerouted = None
        self._out = None

    @property
    def units(self):
        return sum(self.sizes)

    def enqueue(self):
        """Launch only (no host synchronisation)."""
        if self.plan is not None:
            self.plan.enqueue()

    def _dense(self, which, rest):
        """The dense scan of the walkers ``rest[i]`` of the orders ``which``, per order, in calls of at most SCAN_MAX_CAND candidates."""
        out = []
        for i in which:
            parts = [self.orders[i].local_scan(self.mds[i], self.rows[i][rest[i]], self.cands[i][q:q + SCAN_MAX_CAND], self.max_units)
                     for q in range(0, len(self.cands[i]), SCAN_MAX_CAND)]
            res = dict(lnl=parts[0]["lnl"], info=parts[0]["info"])
            res.update({key: np.concatenate([p[key] for p in parts], axis=1) for key in ("quad", "trace", "fisher")})
            out.append(res)
        return out

    def _rest(self, infos):
        rest = rerouted_units(self.fits, infos, self.solver)
        self.rerouted = sum(len(idx) for idx in rest)
        return rest

    def collect(self):
        """Per order a dict of numpy arrays: quad, trace, fisher (B, n_i), lnl (B,), info (B,); refused units have ``-inf``, NaN
        and INFO_BANDWIDTH."""
        outs = [refused_output(n, {key: (len(c),) for key in ("quad", "trace", "fisher")}) for n, c in zip(self.sizes, self.cands)]
        if self.plan is not None:
            for i, got in zip(self.on_device, self.plan.collect()):
                for key, v in got.items():
                    outs[i][key][self.idx[i]] = v
        internal = sum(int(np.count_nonzero(o["info"] == INFO_INTERNAL)) for o in outs)
        if internal:
            import warnings

            warnings.warn(f"banded solver: internal status -5 for {internal} unit(s); recomputed densely", RuntimeWarning,
                          stacklevel=2)
        rest = self._rest([o["info"] for o in outs])
        which = [i for i, idx in enumerate(rest) if len(idx)]
        if which:
            merge_units(outs, rest, self._dense(which, rest))
        self._out = outs
        return outs

    def mean(self):
        """Per order ``(z_mean, amp_mean, count)``: ``z = U / sqrt(fisher)`` and ``amp = U / fisher``, ``U = (quad - trace) / 2``,
        averaged over the ``count`` walkers that evaluate in that order.  An order whose units all ran on the band kernels is
        averaged on the device (sf_local_scan_mean: only the means are copied to the host); an order with a refused or re-routed
        unit by the same rule on the host (:func:`scan_mean_host`) from the collected triples."""
        infos = [np.full(n, INFO_BANDWIDTH, dtype=np.int32) for n in self.sizes]
        if self.plan is not None:
            codes = self.plan.info.cpu().numpy()
            ends = np.cumsum(self.plan.sizes)
            for k, i in enumerate(self.on_device):
                infos[i][self.idx[i]] = codes[ends[k] - self.plan.sizes[k]:ends[k]]
        rest = self._rest(infos)
        on_device = {i: k for k, i in enumerate(self.on_device)}
        host = [i for i in range(len(self.sizes)) if len(rest[i]) or i not in on_device or not self.fits[i].all()]
        outs = self.collect() if host else None
        means = []
        for i in range(len(self.sizes)):
            if i in host:
                means.append(scan_mean_host(outs[i]["quad"], outs[i]["trace"], outs[i]["fisher"], outs[i]["info"]))
            else:
                means.append(self.plan.mean(on_device[i]))
        return means


def local_scan_banded_multi(orders, mds, rows_list, cands, solver="banded", max_units=None, sync=True):
    """The score scan for new local kernels for the (order x walker) units of several orders of ONE device on the band solver
    (:class:`BandedMultiScanPlan`; ``solver``: "banded" or "auto").  Returns its per-order dicts; with ``sync=False`` the
    un-synchronised plan (``plan.collect()`` or ``plan.mean()`` later)."""
    plan = BandedMultiScanPlan(orders, mds, rows_list, cands, solver=solver, max_units=max_units)
    plan.enqueue()
    return plan.collect() if sync else plan
