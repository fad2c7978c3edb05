"""
Multi-order model: the sum of independent per-order log-likelihoods.

The reference ships only a stub (``class EchelleModel: pass``, Starfish/models/echelle_model.py:1-2;
multi-order fitting "will be added back", docs/conversion.rst:7-8).  Orders are statistically
independent given the stellar parameters (docs/intro.rst:71-73), so lnL = sum over orders; each
order is a :class:`SpectrumModel` whose (walker x order) units are evaluated in batched device passes
and may live on different GPUs (``devices``) with only a host-side sum -- no collective.
"""
import re

import numpy as np

from .._flatdict import FlatterDict
from ..spectrum import Spectrum
from .spectrum_model import SpectrumModel

#: top-level parameters that may be sampled per order (flux calibration, noise model, velocity, broadening,
#: extinction); the emulator grid parameters are always shared
PER_ORDER_PARAMS = ("cheb", "log_scale", "global_cov", "local_cov", "vz", "vsini", "Av")
_PREFIXED = re.compile(r"order(\d+):(.+)$")


class EchelleModel:
    def __init__(self, emulator, data, grid_params, devices=None, name="EchelleModel", solver="dense", per_order=None,
                 **params):
        """``params`` are the starting values of every order (vz, vsini, log_scale, global_cov, cheb, ...);
        per-order overrides can be set afterwards on ``self.orders[i]``.  ``solver`` as in
        :class:`SpectrumModel`: "dense" (the reference's algorithm: all (order x walker) units in one batched
        Cholesky), "auto" / "banded" (band + rank-m Woodbury per order, same value to rounding).
        ``per_order``: names from :data:`PER_ORDER_PARAMS` that every order samples on its own (labels
        ``order{i}:<name>...``, after the shared labels); None: every parameter is shared."""
        self.name = name
        self.orders = []
        for i, order in enumerate(data):
            single = Spectrum(order._wave, order._flux, order._sigma, order.mask, name=f"{data.name}[{i}]")
            dev = None if devices is None else devices[i % len(devices)]
            kw = {k: (dict(v) if isinstance(v, dict) else ([dict(x) for x in v] if k == "local_cov" else
                       (list(v) if isinstance(v, (list, tuple)) else v))) for k, v in params.items()}
            self.orders.append(SpectrumModel(emulator, single, grid_params, device=dev, name=f"{name}[{i}]", solver=solver, **kw))
        self.per_order = self._check_per_order(per_order, self.orders)

    @classmethod
    def from_orders(cls, models, name="EchelleModel", per_order=None):
        """Assemble from existing per-order :class:`SpectrumModel` objects (e.g. one emulator chunk per order,
        per-order frozen local kernels).  Without ``per_order`` all orders must expose the same thawed labels;
        with it only the shared ones (values from order 0), the per-order groups may differ in membership too."""
        self = cls.__new__(cls)
        self.name = name
        self.orders = list(models)
        if not self.orders:
            raise ValueError("EchelleModel needs at least one order")
        self.per_order = self._check_per_order(per_order, self.orders)
        if self.per_order is None:
            labels = self.orders[0].labels
            for m in self.orders[1:]:
                if m.labels != labels:
                    raise ValueError(f"orders disagree on the thawed parameters: {m.labels} vs {labels}")
        else:
            self._layout()  # (raises if the shared labels disagree)
        return self

    @staticmethod
    def _check_per_order(per_order, orders):
        if per_order is None:
            return None
        names = tuple(str(n) for n in np.atleast_1d(per_order))
        grid = set(orders[0].emulator.param_names) if orders else set()
        for n in names:
            if n in grid:
                raise ValueError(f"{n!r} is an emulator grid parameter: those are shared by every order")
            if n not in PER_ORDER_PARAMS:
                raise ValueError(f"{n!r} cannot be sampled per order (one of {', '.join(PER_ORDER_PARAMS)})")
        return names

    def _is_per_order(self, key):
        return self.per_order is not None and key.split(":", 1)[0] in self.per_order

    def _order_of(self, name):
        """``order{i}:<key>`` -> (i, key); None for a bare name."""
        hit = _PREFIXED.match(name)
        if not hit:
            return None
        i, key = int(hit.group(1)), hit.group(2)
        if not 0 <= i < len(self.orders):
            raise ValueError(f"{name}: the model has {len(self.orders)} orders")
        if not self._is_per_order(key):
            raise ValueError(f"{name}: {key!r} is not a per-order parameter of this model")
        return i, key

    def _layout(self):
        """(labels, cols): the model's labels, and for every order the columns of a parameter vector that hold
        that order's own labels (shared labels first, then each order's per-order labels, prefixed).  Without
        ``per_order``: order 0's labels and every column for every order, whatever the other orders' labels are."""
        if self.per_order is None:
            labels = tuple(self.orders[0].labels)
            return labels, [np.arange(len(labels), dtype=np.intp)] * len(self.orders)
        shared = [k for k in self.orders[0].labels if not self._is_per_order(k)]
        labels, cols = list(shared), []
        for i, m in enumerate(self.orders):
            own = m.labels
            mine = [k for k in own if not self._is_per_order(k)]
            if mine != shared:
                raise ValueError(f"order {i} disagrees with order 0 on the shared thawed parameters: {mine} vs {shared}")
            c = []
            for k in own:
                if self._is_per_order(k):
                    c.append(len(labels))
                    labels.append(f"order{i}:{k}")
                else:
                    c.append(shared.index(k))
            cols.append(np.array(c, dtype=np.intp))
        return tuple(labels), cols

    def __len__(self):
        return len(self.orders)

    def _side_streams(self, device, n=4):
        import torch

        pools = self.__dict__.setdefault("_streams", {})
        key = str(device)
        if key not in pools:
            pools[key] = [torch.cuda.Stream(device=device) for _ in range(n)]
        return pools[key]

    @property
    def labels(self):
        if self.per_order is None:
            return self.orders[0].labels
        return self._layout()[0]

    def _route(self, op, names):
        names = [str(n) for n in np.atleast_1d(names)]
        if self.per_order is None or names[0] == "all":
            for m in self.orders:
                getattr(m, op)(names)
            return
        for name in names:
            hit = self._order_of(name)
            if hit is not None:  # one order's parameter or group
                getattr(self.orders[hit[0]], op)(hit[1])
                continue
            targets = [m for m in self.orders if name in m.params] or self.orders
            for m in targets:
                getattr(m, op)(name)

    def freeze(self, names):
        """As :meth:`SpectrumModel.freeze` on every order; a prefixed name (``order3:cheb:2``, ``order1:local_cov``)
        acts on that order only."""
        self._route("freeze", names)

    def thaw(self, names):
        """As :meth:`SpectrumModel.thaw` on every order; a prefixed name acts on that order only."""
        self._route("thaw", names)

    def get_param_vector(self):
        if self.per_order is None:
            return self.orders[0].get_param_vector()
        labels, cols = self._layout()
        out = np.empty(len(labels))
        for i in reversed(range(len(self.orders))):  # (shared values: order 0's)
            out[cols[i]] = self.orders[i].get_param_vector()
        return out

    def set_param_vector(self, P):
        if self.per_order is None:
            for m in self.orders:
                m.set_param_vector(P)
            return
        labels, cols = self._layout()
        P = np.asarray(P, dtype=np.float64)
        if len(P) != len(labels):
            raise ValueError("Param Vector does not match length of thawed parameters")
        for m, c in zip(self.orders, cols):
            m.set_param_vector(P[c])

    def get_param_dict(self, flat=False):
        """Thawed parameters under :attr:`labels` (shared ones from order 0), nested or flat."""
        out = FlatterDict()
        own = [m.get_param_dict(flat=True) for m in self.orders]
        for key, val in own[0].items():
            if not self._is_per_order(key):
                out[key] = val
        for i, d in enumerate(own):
            for key, val in d.items():
                if self._is_per_order(key):
                    out[f"order{i}:{key}"] = val
        return out if flat else out.as_dict()

    def set_param_dict(self, params):
        """Update parameters: a prefixed key goes to its order, a bare key to every order that has it."""
        for key, val in FlatterDict(params).items():
            hit = self._order_of(key)
            if hit is not None:
                self.orders[hit[0]].set_param_dict({hit[1]: val})
                continue
            targets = [m for m in self.orders if key in m.params]
            if not targets:
                raise KeyError(f"{key} is not a parameter of any order")
            for m in targets:
                m.set_param_dict({key: val})

    def _prior_terms(self, priors):
        """(prior, order index, key in that order) of every prior term: keys are looked up as the reference does
        (``key in params``); a prefixed key is its order's, a bare per-order key counts once per order that has it,
        a shared key once (order 0's)."""
        terms = []
        for key, prior in (priors or {}).items():
            hit = _PREFIXED.match(key)
            if hit and self._is_per_order(hit.group(2)):
                i, k = int(hit.group(1)), hit.group(2)
                if i < len(self.orders) and k in self.orders[i].params:
                    terms.append((prior, i, k))
            elif self._is_per_order(key):
                terms += [(prior, i, key) for i, m in enumerate(self.orders) if key in m.params]
            elif key in self.orders[0].params:
                terms.append((prior, 0, key))
        return terms

    def _batch_prior(self, P, priors, cols):
        """Log-prior of every row of ``P`` (:attr:`labels` order); parameters not sampled use the current value."""
        lp = np.zeros(P.shape[0])
        for prior, i, key in self._prior_terms(priors):
            own = self.orders[i].labels
            if key in own:
                lp += np.asarray(prior.logpdf(P[:, cols[i][own.index(key)]]), dtype=np.float64)
            else:
                lp += prior.logpdf(self.orders[i][key])
        return lp

    @staticmethod
    def _by_device(packed):
        """The orders of ``packed`` (``_pack`` results) that may share one multi-order call: lists of indices, one per
        device and emulator shape."""
        groups = {}
        for idx, (dev, _md, _rows) in enumerate(packed):
            groups.setdefault((str(dev.dev), dev.m, dev.P), []).append(idx)
        return list(groups.values())

    def log_likelihood(self, priors=None):
        """Sum of the per-order likelihoods; the prior is counted once (per order for a per-order parameter)."""
        if self.per_order is None:
            total = self.orders[0].log_likelihood(priors)
            for m in self.orders[1:]:
                total += m.log_likelihood(None)
            return total
        lp = 0.0
        for prior, i, key in self._prior_terms(priors):
            lp += prior.logpdf(self.orders[i][key])
        if not np.isfinite(lp):
            return -np.inf
        return sum(m.log_likelihood(None) for m in self.orders) + lp

    def log_likelihood_batch(self, P, priors=None, return_info=False, return_orders=False):
        """lnL (B,) for B parameter vectors (rows of ``P`` in :attr:`labels` order; every order gets the columns of
        its own labels).  All (order x walker) units of a device are evaluated in ONE enqueue
        (``sf_loglike_multi_batch``, or ``sf_loglike_multi_batch_md`` when the orders' row layouts differ: every
        order fills its own covariance matrices, all of them share one batched Cholesky) with one host
        synchronisation per device; devices work concurrently.  The sum over orders happens on the host (no
        collective).  Walkers that fail in any order get ``-inf``; ``info`` is the first non-zero per-order code.
        With ``return_orders`` the (n_orders, B) per-order values are returned too."""
        from .. import _multi as M

        P = np.atleast_2d(np.asarray(P, dtype=np.float64))
        B = P.shape[0]
        labels, cols = self._layout()
        if P.shape[1] != len(labels):
            raise ValueError("Param Vector does not match length of thawed parameters")
        order_P = [P[:, c] for c in cols]
        prior_lp = self._batch_prior(P, priors, cols)
        finite = np.isfinite(prior_lp)
        lnl = np.full(B, -np.inf)
        info = np.zeros(B, dtype=np.int32)
        per_order = np.full((len(self.orders), B), -np.inf)
        structured = any(m.solver != "dense" for m in self.orders)
        vals = np.zeros((len(self.orders), int(finite.sum())))  # per order, of the walkers with a finite prior
        codes = np.zeros((len(self.orders), int(finite.sum())), dtype=np.int32)

        def reduce_orders():
            per_order[:, finite] = vals
            lnl[finite] = vals.sum(axis=0) + prior_lp[finite]
            bad = codes != 0
            info[finite] = np.where(bad.any(axis=0), codes[bad.argmax(axis=0), np.arange(codes.shape[1])], 0)

        if finite.any() and structured:
            # structure-exploiting solver: one banded call per order (a few ms each instead of a share of the dense
            # batch; orders may need different half-widths, so they are not merged)
            # every order is enqueued before anything is waited for; the orders of a device take turns on a few
            # side streams (a banded call of 64 walkers fills half of the chip) -- ONE synchronisation per device
            import torch

            pending, used = [], {}
            for i, m in enumerate(self.orders):
                dev, md, rows = m._pack(order_P[i][finite], update_caches=False)
                if m.solver == "dense":
                    pending.append((i, dev, md, None, rows))
                    continue
                pool = self._side_streams(dev.dev)
                st = pool[len(used.setdefault(str(dev.dev), [])) % len(pool)]
                used[str(dev.dev)].append(st)
                st.wait_stream(torch.cuda.current_stream(dev.dev))
                with torch.cuda.stream(st):
                    pending.append((i, dev, md, dev.structured_enqueue(md, rows), rows))
            for key in used:
                torch.cuda.synchronize(torch.device(key))
            for i, dev, md, pend, rows in pending:
                out = dev.loglike(md, rows) if pend is None else dev.structured_collect(md, pend, self.orders[i].solver)
                vals[i] = np.where(out["info"] == 0, out["lnl"], -np.inf)
                codes[i] = out["info"]
            reduce_orders()
        elif finite.any():
            packed = [m._pack(order_P[i][finite], update_caches=False) for i, m in enumerate(self.orders)]
            # one multi-order call per device (and emulator shape): orders whose row layouts differ -- per-order
            # Chebyshev terms, another number of local kernels, ... -- pass one descriptor each
            pending = []
            for idxs in self._by_device(packed):  # enqueue everything first, synchronise afterwards
                devs = [packed[i][0] for i in idxs]
                mds = [packed[i][1] for i in idxs]
                same = all(M.model_desc_key(m) == M.model_desc_key(mds[0]) for m in mds)
                pending.append((idxs, M.loglike_multi(devs, mds[0] if same else mds, [packed[i][2] for i in idxs],
                                                      sync=False)))
            for idxs, plan in pending:
                for i, out in zip(idxs, plan.collect()):
                    vals[i] = out["lnl"]
                    codes[i] = out["info"]
            reduce_orders()
        self.last_info = info
        out = (lnl,)
        if return_info:
            out += (info,)
        if return_orders:
            out += (per_order,)
        return out if len(out) > 1 else lnl

    # ------------------------------------------------------------------ likelihood gradient of all orders in one pass
    def _gradient_layout(self, solver=None):
        """Host logic of the gradient, no device: ``(labels, cols, requests, sources)``.  ``solver``: None -- every order's
        own ``solver`` must be "dense"; "dense", "banded" or "auto" -- the solver of the gradient call, whatever the orders'
        own is (anything else: the ``ValueError`` of :func:`starfish_amd._runtime.check_solver`).  ``cols[i]``: the columns of a
        parameter vector that hold order i's own labels; ``requests[i] = (mean_columns, want_cov)``: what order i asks the
        device for (:class:`starfish_amd._multi.MultiGradPlan`); ``sources[j]``: the ``(order, slot)`` pairs of the
        per-unit gradient rows that label j adds up, ascending in the order -- a unit's row holds its order's mean slots in
        :attr:`SpectrumModel.mean_gradient_labels` order, then all covariance slots of its descriptor.  A shared label has a
        source in every order, an ``order{i}:`` label one, ``Rv`` none.  Raises ``ValueError``, naming the order, for what
        the device does not differentiate."""
        from .. import _device as D

        if solver is not None:
            D.check_solver(solver, or_none=True)
        labels, cols = self._layout()
        if not labels:
            raise ValueError("no thawed parameter to differentiate in")
        requests, sources = [], [[] for _ in labels]
        for i, m in enumerate(self.orders):
            if solver is None and m.solver != "dense":
                raise ValueError(f"order {i}: the gradient runs on the dense solver only, not solver={m.solver!r}")
            md = m._model_desc(None)
            own, mean, cov = list(m.labels), m.mean_gradient_labels, m.gradient_labels
            try:
                columns = m._mean_gradient_columns(None, md) if mean else []
            except ValueError as e:
                raise ValueError(f"order {i}: {e}") from None
            if len(columns) > D.MEAN_GRAD_MAX_SLOTS:
                raise ValueError(f"order {i}: {len(columns)} thawed mean-flux parameters, the device differentiates in at most "
                                 f"{D.MEAN_GRAD_MAX_SLOTS} per order")
            requests.append((columns, bool(cov)))
            for k, key in enumerate(mean):
                sources[cols[i][own.index(key)]].append((i, k))
            for key, slot in zip(cov, m._gradient_slots(md)):
                sources[cols[i][own.index(key)]].append((i, len(columns) + slot))
        return labels, cols, requests, sources

    def log_likelihood_gradient_batch(self, P, return_info=False, return_orders=False, solver=None):
        """``(lnL (B,), grad (B, len(labels)))`` for B parameter vectors (rows of ``P`` in :attr:`labels` order), no priors:
        the sum of the per-order likelihoods and its analytic gradient in every thawed label, from ONE factorisation per
        (order x walker) unit and one enqueue per device (``sf_loglike_multi_grad_batch_md``).  A shared label receives the
        sum over the orders that have it, an ``order{i}:`` label order i's column, a thawed ``Rv`` a zero column.  The sum over
        the orders runs in ascending order index -- on the device (``sf_multi_grad_reduce``) when all orders share one
        call, on the host by the same rule when they live on several devices.  Walkers that fail in any order get
        ``-inf`` and a NaN row; ``info`` is the first non-zero per-order code.  With ``return_orders`` the (n_orders, B)
        per-order likelihoods are returned too.  The model's own state is not modified.

        solver: None    -- the dense call above; every order's own ``solver`` must be "dense";
                "dense" -- the same call, whatever the orders' own ``solver`` is;
                "banded" -- the band + Woodbury solver, all units of a device in one launch sequence
                            (``sf_loglike_banded_multi_grad_batch_md``): agrees with the dense call to rounding, not bit for
                            bit; a walker with a unit whose covariance support exceeds the LDS window gets ``-inf``, a NaN
                            row and info = -4;
                "auto"  -- banded for the units whose half-width bound fits the window, the dense call for the rest."""
        from .. import _multi as M

        labels, cols, requests, sources = self._gradient_layout(solver)
        banded = solver in ("banded", "auto")
        P = np.atleast_2d(np.asarray(P, dtype=np.float64))
        if P.shape[1] != len(labels):
            raise ValueError("Param Vector does not match length of thawed parameters")
        B = P.shape[0]
        packed = [m._pack(P[:, cols[i]], update_caches=False) for i, m in enumerate(self.orders)]
        pending = []
        for idxs in self._by_device(packed):  # enqueue everything first, synchronise afterwards
            if not any(requests[i][0] or requests[i][1] for i in idxs):  # nothing thawed in these orders: lnl only
                pending.append((idxs, M.loglike_multi([packed[i][0] for i in idxs], [packed[i][1] for i in idxs],
                                                      [packed[i][2] for i in idxs], sync=False)))
                continue
            call, kw = (M.loglike_banded_multi_grad, dict(solver=solver)) if banded else (M.loglike_multi_grad, {})
            pending.append((idxs, call([packed[i][0] for i in idxs], [packed[i][1] for i in idxs],
                                       [packed[i][2] for i in idxs], [requests[i] for i in idxs], sync=False, **kw)))
        unit_lnl = np.full((len(self.orders), B), -np.inf)
        unit_info = np.zeros((len(self.orders), B), dtype=np.int32)
        unit_grad = [np.zeros((B, 0))] * len(self.orders)
        for idxs, plan in pending:
            for i, out in zip(idxs, plan.collect()):
                unit_lnl[i], unit_info[i] = out["lnl"], out["info"]
                unit_grad[i] = out.get("grad", unit_grad[i])
        if len(pending) == 1 and isinstance(pending[0][1], (M.MultiGradPlan, M.BandedMultiGradPlan)):
            lnl, grad, info = pending[0][1].reduce(sources)
        else:
            lnl, grad, info = M.reduce_orders_host(unit_lnl, unit_info, unit_grad, sources)
        self.last_info = info
        out = (lnl, grad)
        if return_info:
            out += (info,)
        if return_orders:
            out += (np.where(unit_info == 0, unit_lnl, -np.inf),)
        return out

    def log_likelihood_gradient(self, solver=None):
        """``(lnL, {label: d lnL / d label})`` of the current state, no priors.  Raises as
        :meth:`SpectrumModel.log_likelihood` does for a point the device flags; the model's state is not modified.
        ``solver`` as for :meth:`log_likelihood_gradient_batch`."""
        extra = {} if solver is None else dict(solver=solver)
        lnl, grad, info = self.log_likelihood_gradient_batch(self.get_param_vector()[None, :], return_info=True, **extra)
        SpectrumModel._raise_for_info(info[0])
        return float(lnl[0]), dict(zip(self.labels, (float(v) for v in grad[0])))

    # ------------------------------------------------------------------ Fisher information of all orders in one pass
    @property
    def mean_gradient_labels(self):
        """tuple of str : the labels of :attr:`labels` that are not under ``global_cov:`` / ``local_cov:`` (bare or behind
        ``order{i}:``) and are not ``Rv``, in :attr:`labels` order: the parameters of :meth:`fisher_information`."""
        def bare(key):
            hit = _PREFIXED.match(key)
            return hit.group(2) if hit else key

        return tuple(key for key in self.labels if not bare(key).startswith(("global_cov:", "local_cov:")) and bare(key) != "Rv")

    def _fisher_layout(self, solver=None):
        """Host logic of the Fisher matrix, no device, in the manner of :meth:`_gradient_layout`: ``(labels, cols, columns,
        sources)``.  ``solver`` as there.  ``columns[i]``: the columns of order i's C-ABI parameter row that hold its mean-flux
        labels (:attr:`SpectrumModel.mean_gradient_labels` order); ``sources[j]``: the ``(order, slot)`` pairs of the unit
        matrices that label j of :attr:`mean_gradient_labels` adds up, ascending in the order -- a shared label has a source in
        every order, an ``order{i}:`` label one.  Raises ``ValueError``, naming the order, for what the device does not
        differentiate, for more than ``MEAN_GRAD_MAX_SLOTS`` columns in one order and, with ``solver=None``, for an order whose
        own solver is not "dense"."""
        from .. import _device as D

        if solver is not None:
            D.check_solver(solver, or_none=True)
        labels, cols = self._layout()
        mean = self.mean_gradient_labels
        if not mean:
            raise ValueError("no thawed mean-flux parameter to take the Fisher information in")
        position = {labels.index(key): j for j, key in enumerate(mean)}
        columns, sources = [], [[] for _ in mean]
        for i, m in enumerate(self.orders):
            if solver is None and m.solver != "dense":
                raise ValueError(f"order {i}: solver=None runs the Fisher information on the dense solver only, not "
                                 f"solver={m.solver!r}; pass solver=")
            own = list(m.labels)
            try:
                c = m._mean_gradient_columns(None, m._model_desc(None))
            except ValueError as e:
                raise ValueError(f"order {i}: {e}") from None
            if len(c) > D.MEAN_GRAD_MAX_SLOTS:
                raise ValueError(f"order {i}: {len(c)} thawed mean-flux parameters, the device takes the Fisher information in at "
                                 f"most {D.MEAN_GRAD_MAX_SLOTS} per order")
            columns.append(c)
            for k, key in enumerate(m.mean_gradient_labels):
                sources[position[int(cols[i][own.index(key)])]].append((i, k))
        return labels, cols, columns, sources

    def fisher_information_batch(self, P, return_info=False, return_orders=False, solver=None):
        """The Fisher information of the mean-flux parameters at fixed covariance for B parameter vectors (rows of ``P`` in
        :attr:`labels` order; covariance labels take their values from ``P``): ``(B, p, p)`` in :attr:`mean_gradient_labels`
        order, symmetric bit for bit -- the sum over the orders of every order's ``F_ij = fdot_i^T C^-1 fdot_j``
        (:meth:`SpectrumModel.fisher_information`), embedded by the labels: a shared label adds up all orders, the entry between
        labels of two different orders is exactly 0.  This is the Gauss-Newton, fixed-covariance matrix: the term ``1/2 tr(C^-1
        dC_i C^-1 dC_j)`` that a grid parameter has because the emulator's rows sit inside the covariance is left out, and so is
        the block of the covariance hyper-parameters (the mean / covariance cross block of a Gaussian's Fisher matrix is zero):
        a single order has it from :meth:`SpectrumModel.covariance_fisher_information`, a one-pass multi-order call does not exist.
        A walker that fails in any order gets a NaN matrix; with ``return_info`` ``(fisher, info)``, ``info`` the first non-zero
        per-order code; with ``return_orders`` also the list of the per-order unit matrices ``(B, p_i, p_i)``.  The model's
        state is not modified.

        solver: None / "dense" -- every order's dense ``fisher_mean`` call (None: every order's own ``solver`` must be "dense");
                "banded" -- the band + Woodbury solver, ONE sweep per (order x walker) unit and all units of a device in one
                            launch sequence (``sf_fisher_banded_multi_batch_md``); a walker with a unit whose covariance
                            support exceeds the LDS window at the call's row count gets a NaN matrix and info = -4;
                "auto"  -- banded for the units whose half-width bound fits that window, the dense call for the rest.
        The sum over the orders runs in ascending order index, on the device (``sf_multi_fisher_reduce``) when one band call
        held every unit, else on the host by the same rule (:func:`starfish_amd._multi.reduce_fisher_host`)."""
        from .. import _multi as M

        labels, cols, columns, sources = self._fisher_layout(solver)
        P = np.atleast_2d(np.asarray(P, dtype=np.float64))
        if P.shape[1] != len(labels):
            raise ValueError("Param Vector does not match length of thawed parameters")
        packed = [m._pack(P[:, cols[i]], update_caches=False) for i, m in enumerate(self.orders)]
        pending = []
        for idxs in self._by_device(packed):  # enqueue everything first, synchronise afterwards
            plan = None
            if solver in ("banded", "auto"):
                plan = M.fisher_banded_multi([packed[i][0] for i in idxs], [packed[i][1] for i in idxs],
                                             [packed[i][2] for i in idxs], [columns[i] for i in idxs], solver=solver, sync=False)
            pending.append((idxs, plan))
        unit = [None] * len(self.orders)
        for idxs, plan in pending:
            outs = plan.collect() if plan is not None else [packed[i][0].fisher_mean(packed[i][1], packed[i][2], columns[i])
                                                            for i in idxs]
            for i, out in zip(idxs, outs):
                unit[i] = out
        if len(pending) == 1 and pending[0][1] is not None:
            _lnl, fisher, info = pending[0][1].reduce(sources)
        else:
            _lnl, fisher, info = M.reduce_fisher_host(np.stack([u["lnl"] for u in unit]), np.stack([u["info"] for u in unit]),
                                                      [u["fisher"] for u in unit], sources)
        self.last_info = info
        out = (fisher,)
        if return_info:
            out += (info,)
        if return_orders:
            out += ([u["fisher"] for u in unit],)
        return out if len(out) > 1 else fisher

    def fisher_information(self, solver=None):
        """:meth:`fisher_information_batch` at the current state: ``(p, p)`` in :attr:`mean_gradient_labels` order -- the
        Gauss-Newton, fixed-covariance matrix, without the ``1/2 tr(C^-1 dC_i C^-1 dC_j)`` term of the grid parameters and without
        the block of the covariance hyper-parameters.  Raises as :meth:`log_likelihood` does for a point the device flags; the
        model's state is not modified."""
        fisher, info = self.fisher_information_batch(self.get_param_vector()[None, :], return_info=True, solver=solver)
        SpectrumModel._raise_for_info(info[0])
        return fisher[0]

    def parameter_covariance(self, priors=None, solver=None):
        """The Laplace covariance of the labels of :attr:`mean_gradient_labels` at the current state (the point :meth:`train`
        found): the inverse of :meth:`fisher_information` plus, for every prior on one of these labels, ``-d^2 logpdf / d
        label^2`` by a central second difference with step ``eps^(1/3) max(1, |x|)``.  ``priors`` are looked up as :meth:`train`
        does: a bare per-order key counts once per order, on that order's own label.  The covariance hyper-parameters are held
        fixed; see :meth:`fisher_information_batch` for what the matrix leaves out.  Inverted in normalised form by Cholesky; a
        matrix that is not positive definite raises ``np.linalg.LinAlgError`` naming the labels
        (:func:`starfish_amd._map.laplace_covariance`)."""
        from .. import _map

        for key, prior in (priors or {}).items():
            if not callable(getattr(prior, "logpdf", None)):
                raise ValueError(f"Invalid priors. {key} does not have a `logpdf` method")
        labels, cols = self._layout()
        mean = self.mean_gradient_labels
        terms = []
        for prior, i, key in self._prior_terms(priors):
            own = self.orders[i].labels
            if key in own and labels[cols[i][own.index(key)]] in mean:
                terms.append((mean.index(labels[cols[i][own.index(key)]]), prior, float(self.orders[i][key])))
        return _map.laplace_covariance(self.fisher_information(solver=solver), mean, terms)

    # ------------------------------------------------------------------ where do new local kernels belong, in every order?
    def _scan_inputs(self, mus, sigmas, wl_range, solver=None):
        """Host logic of the scan, no device work: per order ``(mus_i, sigmas_i, cand_i)`` as
        :meth:`SpectrumModel._scan_candidates` checks them, or None for an order that ``wl_range`` leaves without a centre.
        ``mus``: None -- every order's own pixels; else one array of centres per order.  ``sigmas``: None -- the default widths;
        widths (km/s) shared by the orders; or one list of widths per order.  ``solver``: None -- every order's own ``solver`` must
        be "dense"; under "banded" a candidate whose patch is wider than the band solver's limit is a ``ValueError``.  Every
        ``ValueError`` names the order."""
        from .. import _device as D
        from ._diagnostics import DEFAULT_SCAN_SIGMAS

        if solver is not None:
            D.check_solver(solver, or_none=True)
        n = len(self.orders)
        if mus is not None and len(mus) != n:
            raise ValueError(f"mus: {len(mus)} lists of centres for {n} orders (None: every order's own pixels)")
        sigmas = DEFAULT_SCAN_SIGMAS if sigmas is None else sigmas
        per_order = not np.isscalar(sigmas) and len(sigmas) > 0 and np.ndim(sigmas[0]) > 0
        if per_order and len(sigmas) != n:
            raise ValueError(f"sigmas: {len(sigmas)} lists of widths for {n} orders (or one list shared by all)")
        out = []
        for i, m in enumerate(self.orders):
            if solver is None and m.solver != "dense":
                raise ValueError(f"order {i}: solver=None runs the scan on the dense solver only, not solver={m.solver!r}; pass "
                                 f"solver=")
            centres = np.asarray(m.data.wave if mus is None else mus[i], dtype=np.float64).ravel()
            if wl_range is not None:
                centres = centres[(centres >= wl_range[0]) & (centres <= wl_range[1])]
            if not centres.size:
                out.append(None)
                continue
            limit = None
            if solver == "banded":  # (a size query of the order's context; nothing is enqueued)
                dev, md, _ = m._pack(None, update_caches=False)
                limit = dev.local_scan_banded_max_patch(md)
            try:
                out.append(m._scan_candidates(centres, sigmas[i] if per_order else sigmas, None, limit))
            except ValueError as e:
                raise ValueError(f"order {i}: {e}") from None
        return out

    @staticmethod
    def _scan_result(out, nsig, nmu):
        """The dict of :meth:`SpectrumModel.local_kernel_scan_batch` from a device scan's quad, trace, fisher (B, nsig * nmu)."""
        shape = (out["quad"].shape[0], nsig, nmu)
        quad, trace, fisher = (np.asarray(out[key]).reshape(shape) for key in ("quad", "trace", "fisher"))
        score = 0.5 * (quad - trace)
        with np.errstate(divide="ignore", invalid="ignore"):
            z = np.where(fisher == 0, np.nan, score / np.sqrt(fisher))
            amp = np.where(fisher == 0, np.nan, score / fisher)
        return {"score": score, "information": fisher, "z": z, "amp": amp, "quad": quad, "trace": trace}

    def _scan_run(self, P, inputs, solver, mean=False):
        """The device side of the scan for the orders of ``inputs`` that have candidates: per order (None: skipped) the scan's
        dict (quad, trace, fisher (B, ncand_i), lnl, info) -- with ``mean`` ``(z_mean, amp_mean, count)`` over the walkers that
        evaluate there instead -- and the (n_orders, B) status codes, 0 for a skipped order."""
        from .. import _multi as M

        labels, cols = self._layout()
        P = np.atleast_2d(np.asarray(P, dtype=np.float64))
        if P.shape[1] != len(labels):
            raise ValueError("Param Vector does not match length of thawed parameters")
        active = [i for i, v in enumerate(inputs) if v is not None]
        packed = {i: self.orders[i]._pack(P[:, cols[i]], update_caches=False) for i in active}
        outs = [None] * len(self.orders)
        codes = np.zeros((len(self.orders), P.shape[0]), dtype=np.int32)
        if solver in ("banded", "auto"):
            pending = []
            for group in self._by_device([packed[i] for i in active]):  # enqueue everything first, synchronise afterwards
                idxs = [active[k] for k in group]
                pending.append((idxs, M.local_scan_banded_multi([packed[i][0] for i in idxs], [packed[i][1] for i in idxs],
                                                                [packed[i][2] for i in idxs], [inputs[i][2] for i in idxs],
                                                                solver=solver, sync=False)))
            for idxs, plan in pending:
                for i, out in zip(idxs, plan.mean() if mean else plan.collect()):
                    outs[i] = out
                    if not mean:
                        codes[i] = out["info"]
            return outs, codes
        for i in active:  # the loop over every order's dense scan
            dev, md, rows = packed[i]
            cand = inputs[i][2]
            parts = [dev.local_scan(md, rows, cand[q:q + M.SCAN_MAX_CAND]) for q in range(0, len(cand), M.SCAN_MAX_CAND)]
            out = dict(lnl=parts[0]["lnl"], info=parts[0]["info"])
            out.update({key: np.concatenate([p[key] for p in parts], axis=1) for key in ("quad", "trace", "fisher")})
            codes[i] = out["info"]
            outs[i] = M.scan_mean_host(out["quad"], out["trace"], out["fisher"], out["info"]) if mean else out
        return outs, codes

    def local_kernel_scan_batch(self, P, mus=None, sigmas=None, wl_range=None, return_info=False, solver=None,
                                return_orders=False):
        """:meth:`SpectrumModel.local_kernel_scan_batch` for every order, for B parameter vectors (rows of ``P`` in :attr:`labels`
        order; every order gets the columns of its own labels): a list with one dict per order -- "score", "information", "z",
        "amp", "quad", "trace" of shape ``(B, len(sigmas), n_centres_i)`` -- the score test for one more local kernel at every
        centre and width, with every kernel the order already has in its covariance.  ``mus``: None -- every order's own pixels;
        else one array of centres per order.  ``wl_range`` = (lo, hi) keeps the centres inside it; an order left without centres
        is skipped, its entry is None.  ``sigmas`` (km/s; None: 8, 15, 30): shared, or one list per order.  With ``return_info``
        ``(results, info)``, ``info`` (B,) the first non-zero per-order code of every walker; with ``return_orders`` also the
        (n_orders, B) per-order codes (0 for a skipped order).  A walker that fails in an order has NaN rows there.  The model's
        state is not modified.

        solver: None / "dense" -- the loop over every order's dense ``local_scan`` (None: every order's own ``solver`` must be
                            "dense");
                "banded" -- the band + Woodbury solver, all (order x walker) units of a device in one launch sequence
                            (``sf_local_scan_banded_multi_batch_md``), everything enqueued before anything is synchronised; a
                            candidate that reaches more pixels than the band solver scans (145 for up to 15 emulator components)
                            is a ``ValueError`` naming the order before any device call; a unit whose covariance support exceeds
                            the LDS window gets NaN rows and info = -4;
                "auto"  -- banded for the units that fit the window, the order's dense scan for the rest and for every unit of an
                            order with a candidate beyond the limit."""
        inputs = self._scan_inputs(mus, sigmas, wl_range, solver)
        outs, codes = self._scan_run(P, inputs, solver)
        res = [None if out is None else self._scan_result(out, len(inp[1]), len(inp[0])) for out, inp in zip(outs, inputs)]
        bad = codes != 0
        info = np.where(bad.any(axis=0), codes[bad.argmax(axis=0), np.arange(codes.shape[1])], 0).astype(np.int32)
        self.last_info = info
        ret = (res,)
        if return_info:
            ret += (info,)
        if return_orders:
            ret += (codes,)
        return ret if len(ret) > 1 else res

    def local_kernel_scan(self, mus=None, sigmas=None, wl_range=None, solver=None):
        """:meth:`local_kernel_scan_batch` at the current state: a list with one dict per order (None for a skipped one) of
        arrays of shape ``(len(sigmas), n_centres_i)``.  Raises as :meth:`log_likelihood` does for a point the device flags; the
        model's state is not modified."""
        res, info = self.local_kernel_scan_batch(self.get_param_vector()[None, :], mus, sigmas, wl_range, return_info=True,
                                                 solver=solver)
        SpectrumModel._raise_for_info(info[0])
        return [None if r is None else {key: v[0] for key, v in r.items()} for r in res]

    def _scan_means(self, P, mus, sigmas, wl_range, solver):
        """What :meth:`propose_local_kernels` picks from: per order None (skipped) or ``(z, amp, mus_i, sigmas_i)`` with ``z`` and
        ``amp`` of shape ``(len(sigmas_i), len(mus_i))`` -- of the current state (``P`` None), or their means over the walkers of
        ``P`` that evaluate in that order: from the device under "banded" / "auto" (``sf_local_scan_mean``), on the host by the
        same rule under None / "dense"."""
        inputs = self._scan_inputs(mus, sigmas, wl_range, solver)
        if P is None:
            outs, codes = self._scan_run(self.get_param_vector()[None, :], inputs, solver)
            for i, out in enumerate(outs):
                if out is not None:
                    SpectrumModel._raise_for_info(codes[i, 0])
            res = [None if out is None else self._scan_result(out, len(inp[1]), len(inp[0])) for out, inp in zip(outs, inputs)]
            return [None if r is None else (r["z"][0], r["amp"][0], inp[0], inp[1]) for r, inp in zip(res, inputs)]
        means, _codes = self._scan_run(P, inputs, solver, mean=True)
        out = []
        for i, (mean, inp) in enumerate(zip(means, inputs)):
            if mean is None:
                out.append(None)
                continue
            z, amp, count = mean
            if not count:
                raise ValueError(f"order {i}: no walker of P evaluates: nothing to average")
            shape = (len(inp[1]), len(inp[0]))
            out.append((z.reshape(shape), amp.reshape(shape), inp[0], inp[1]))
        return out

    def propose_local_kernels(self, threshold=4.0, buffer=None, max_kernels=None, sigmas=None, mus=None, wl_range=None, P=None,
                              solver=None):
        """Where every order's residual asks for local kernels: :meth:`local_kernel_scan` (with ``P``:
        :meth:`local_kernel_scan_batch`, ``z`` and ``amp`` averaged per order over the walkers that evaluate in that order), then
        per order the peak picking of :meth:`SpectrumModel.propose_local_kernels` (``threshold``, ``buffer``; at most
        ``max_kernels`` per order, None: as many as each order can still take).  Returns a list with one list per order (empty for
        a skipped order) of ``{"mu", "log_amp", "log_sigma"}``, sorted by ``mu``.  Raises a ``ValueError`` naming the order if no
        walker of ``P`` evaluates there.  The model is never changed.  ``mus``, ``sigmas``, ``wl_range`` and ``solver`` as for
        :meth:`local_kernel_scan_batch`; under "banded" / "auto" the means over the walkers are taken on the device
        (``sf_local_scan_mean``) and only they are copied to the host.

        The loop that builds the noise model of an echelle spectrum::

            for i, new in enumerate(em.propose_local_kernels(solver="auto")):
                em.orders[i]["local_cov"] = [*em.orders[i]._local_kernels(), *new]
            em.train(gradient_solver="auto")

        and again until nothing is proposed (see :meth:`SpectrumModel.propose_local_kernels` for what the statistic is)."""
        from .. import _device as D
        from ._diagnostics import pick_local_kernels

        picked = []
        for m, got in zip(self.orders, self._scan_means(P, mus, sigmas, wl_range, solver)):
            if got is None:
                picked.append([])
                continue
            z, amp, centres, widths = got
            room = D.MAX_LOCAL - len(m._local_kernels()) if max_kernels is None else max_kernels
            picked.append(pick_local_kernels(z, amp, centres, widths, threshold, buffer, room))
        return picked

    def train(self, priors=None, *, gradient_solver=None, **kwargs):
        """MAP estimate over :attr:`labels`: ``scipy.optimize.minimize(method="L-BFGS-B", jac=True)`` on the analytic gradient
        of :meth:`log_likelihood_gradient_batch` -- a per-order fit has a few hundred parameters, which a simplex search
        cannot handle.  ``priors`` are looked up as :meth:`log_likelihood` does (a bare per-order key counts once per order);
        a prior on an optimised label adds its ``logpdf`` and the slope of it by a central difference with step
        ``eps^(1/3) max(1, |x|)``, priors on other parameters a constant.  A point the device flags raises as
        :meth:`SpectrumModel.log_likelihood` does.  ``kwargs`` go to ``minimize``.  Every evaluation leaves the model at its
        point; a run that succeeds or stops at its iteration limit leaves it at ``soln.x``.  ``gradient_solver``: the
        ``solver`` of :meth:`log_likelihood_gradient_batch` for every evaluation."""
        from .. import _map

        labels, cols, _requests, _sources = self._gradient_layout(gradient_solver)  # (refusals before any device work)
        extra = {} if gradient_solver is None else dict(solver=gradient_solver)
        for key, prior in (priors or {}).items():
            if not callable(getattr(prior, "logpdf", None)):
                raise ValueError(f"Invalid priors. {key} does not have a `logpdf` method")
        terms = self._prior_terms(priors)

        def evaluate(x):
            self.set_param_vector(x)
            lnl, grad, info = self.log_likelihood_gradient_batch(x[None, :], return_info=True, **extra)
            SpectrumModel._raise_for_info(info[0])
            # the priors are added here, not by _map: constant and sampled terms alternate in the order of ``terms``
            value, slope = float(lnl[0]), grad[0].copy()
            for prior, i, key in terms:
                own = self.orders[i].labels
                if key not in own:
                    value += prior.logpdf(self.orders[i][key])
                    continue
                j = cols[i][own.index(key)]
                v, s = _map.prior_value_and_slope(prior, x[j])
                value += v
                slope[j] += s
            return value, slope

        soln = _map.minimize_lbfgsb(evaluate, self.get_param_vector().astype(np.float64), [], None, kwargs,
                                    finite_for="EchelleModel.train")
        if soln.success or soln.status == 1:  # (1: the iteration / evaluation limit; soln.x is the best point so far)
            self.set_param_vector(soln.x)
        return soln
