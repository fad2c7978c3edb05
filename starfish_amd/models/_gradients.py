"""The analytic likelihood gradients of :class:`SpectrumModel` -- in the covariance hyper-parameters, in the mean-flux
parameters, in every thawed label -- and the two L-BFGS-B searches on them (:mod:`starfish_amd._map`)."""
import numpy as np

from .. import _device as D
from .. import _multi as M
from .. import _map
from .. import _rows as R


class Gradients:
    # ------------------------------------------------------------------ gradient in the covariance hyper-parameters
    @property
    def gradient_labels(self):
        """tuple of str : the thawed labels under ``global_cov:`` / ``local_cov:``, in :attr:`labels` order: the parameters
        :meth:`log_likelihood_gradient` differentiates in."""
        return tuple(key for key in self.labels if key.startswith(("global_cov:", "local_cov:")))

    def _gradient_slots(self, md):
        """For every label of :attr:`gradient_labels`, its slot in the device's gradient row
        (:func:`starfish_amd._rows.cov_grad_slot`)."""
        return [R.cov_grad_slot(md, key) for key in self.gradient_labels]

    def _cov_grad_call(self, dev, md, rows, solver):
        """The device call of the covariance gradient; "dense" is the call as it always was."""
        if solver == "dense":
            return dev.loglike_grad(md, rows)
        return dev.loglike_grad(md, rows, solver=solver)

    def log_likelihood_gradient(self, solver=None):
        """``(lnL, {label: d lnL / d label})`` of the current state for the labels of :attr:`gradient_labels`: the analytic
        gradient of :meth:`log_likelihood` (no priors) in the covariance hyper-parameters, from one factorisation
        (Rasmussen & Williams, GPML, eq. 5.9).  In ``mu`` of a local kernel it is the almost-everywhere derivative: the
        likelihood has a kink wherever two pixels of the patch are equidistant from ``mu``.  Raises as
        :meth:`log_likelihood` does; the model's state is not modified.  ``solver``: ``None`` / "dense" the dense factor and the
        support blocks of its inverse, whatever the model's own ``solver`` is; "banded" / "auto" the band + Woodbury solver
        with the band of the inverse by selected inversion (:meth:`DeviceOrder.loglike_grad`)."""
        solver = self._gradient_solver(solver)
        labels = self.gradient_labels
        if not labels:
            raise ValueError("no thawed global_cov / local_cov parameter to differentiate in")
        dev, md, rows = self._pack(update_caches=False)
        out = self._own(self._cov_grad_call(dev, md, rows, solver))
        return float(out["lnl"]), dict(zip(labels, (float(v) for v in out["grad"][self._gradient_slots(md)])))

    def log_likelihood_gradient_batch(self, P, return_info=False, solver=None):
        """:meth:`log_likelihood_gradient` for B walkers (rows of ``P`` in :attr:`labels` order) in one batched device pass:
        ``(lnL (B,), grad (B, len(gradient_labels)))``.  Walkers that fail get ``-inf`` and a NaN row, ``info`` their codes.
        The model's own state is not modified.  ``solver``: as for :meth:`log_likelihood_gradient`."""
        solver = self._gradient_solver(solver)
        if not self.gradient_labels:
            raise ValueError("no thawed global_cov / local_cov parameter to differentiate in")
        P = np.atleast_2d(np.asarray(P, dtype=np.float64))
        dev, md, rows = self._pack(P, update_caches=False)
        out = self._cov_grad_call(dev, md, rows, solver)
        lnl = np.where(out["info"] == 0, out["lnl"], -np.inf)
        grad = out["grad"][:, self._gradient_slots(md)]
        return (lnl, grad, out["info"]) if return_info else (lnl, grad)

    def _prior_split(self, priors, labels):
        """``(sampled, const_lp)`` of :func:`starfish_amd._map.minimize_lbfgsb` for the optimised ``labels``: a prior on
        one of them with its position, in ``labels`` order; priors on other parameters a constant."""
        const_lp = sum(prior.logpdf(self[key]) for key, prior in priors.items() if key in self.params and key not in labels)
        return [(i, priors[key]) for i, key in enumerate(labels) if key in priors], const_lp

    def train_covariance(self, priors=None, *, gradient_solver=None, **kwargs):
        """MAP estimate of the covariance hyper-parameters alone: ``scipy.optimize.minimize(method="L-BFGS-B", jac=True)``
        over :attr:`gradient_labels` with the analytic gradient of :meth:`log_likelihood_gradient_batch`; every other
        parameter keeps its value.  ``priors`` are checked as :meth:`train` checks them; a prior on an optimised label adds
        its ``logpdf`` and the slope of it by a central difference with step ``eps^(1/3) max(1, |x|)`` (scipy's frozen
        distributions expose no derivative), priors on other parameters a constant.  ``gradient_solver``: ``solver`` of
        :meth:`log_likelihood_gradient_batch`.  ``kwargs`` go to ``minimize``.  On success the model is left at ``soln.x``."""
        gradient_solver = self._gradient_solver(gradient_solver)
        priors = self._checked_priors(priors)
        glabels = self.gradient_labels
        if not glabels:
            raise ValueError("no thawed global_cov / local_cov parameter to optimise")
        labels = self.labels
        cols = [labels.index(key) for key in glabels]
        x_all = self.get_param_vector().astype(np.float64)

        def evaluate(x):  # (the model's state is not touched: x goes into a copy of the full vector)
            row = x_all.copy()
            row[cols] = x
            lnl, grad, info = self.log_likelihood_gradient_batch(row[None, :], return_info=True, solver=gradient_solver)
            self._raise_for_info(info[0])
            return lnl[0], grad[0]

        soln = _map.minimize_lbfgsb(evaluate, x_all[cols], *self._prior_split(priors, glabels), kwargs, force_jac=False)
        if soln.success:
            self.set_param_dict(dict(zip(glabels, soln.x)))
        return soln

    # ------------------------------------------------------------------ gradient in the mean-flux parameters
    @property
    def mean_gradient_labels(self):
        """tuple of str : the thawed labels that are not under ``global_cov:`` / ``local_cov:``, in :attr:`labels` order: the
        parameters :meth:`log_likelihood_mean_gradient` differentiates in.  ``Rv`` is left out: it is never passed on."""
        return tuple(key for key in self.labels if not key.startswith(("global_cov:", "local_cov:")) and key != "Rv")

    def _mean_gradient_columns(self, dev, md):
        """For every label of :attr:`mean_gradient_labels`, its column of the C-ABI parameter row; raises ``ValueError`` for a
        model the device does not differentiate."""
        labels = self.mean_gradient_labels
        if not labels:
            raise ValueError("no thawed mean-flux parameter to differentiate in")
        if "log_scale" not in self.params:
            raise ValueError("the mean gradient needs log_scale: the renormalising scale is not differentiated")
        if self.emulator_cov == "paper":
            raise ValueError('the mean gradient covers emulator_cov="code" only, not the form of the paper (emulator_cov="paper")')
        if self.norm and any(key in self.emulator.param_names for key in labels):
            raise ValueError("norm=True with a thawed grid parameter: the derivative of the host's norm-factor interpolant is "
                             "not built; freeze the grid parameters")
        slots = self._slot_of(dev, md)
        return [slots[key] for key in labels]

    @staticmethod
    def _gradient_solver(solver):
        """``solver`` of the gradient methods as :meth:`DeviceOrder.loglike_mean_grad` / ``loglike_grad`` take it.  ``None`` is "dense",
        whatever the model's own ``solver`` is: a model built with ``solver="auto"`` keeps the dense gradient's bits unless the
        caller asks for the band solver."""
        solver = "dense" if solver is None else solver
        D.check_solver(solver, or_none=True)
        return solver

    def _mean_grad_call(self, dev, md, rows, solver):
        """The device call of the mean gradient; "dense" is the call as it always was."""
        columns = self._mean_gradient_columns(dev, md)
        if solver == "dense":
            return dev.loglike_mean_grad(md, rows, columns)
        return dev.loglike_mean_grad(md, rows, columns, solver=solver)

    def log_likelihood_mean_gradient(self, solver=None):
        """``(lnL, {label: d lnL / d label})`` of the current state for the labels of :attr:`mean_gradient_labels`: the analytic
        gradient of :meth:`log_likelihood` (no priors) in vsini, vz, log_scale, Av, the Chebyshev coefficients and the grid
        parameters, from the likelihood's factorisation and one solve with 1 + m right-hand sides.  Raises as
        :meth:`log_likelihood` does; the model's state is not modified.  ``solver``: ``None`` / "dense" the dense factor, "banded" /
        "auto" the band + Woodbury solver with a backward sweep (:meth:`DeviceOrder.loglike_mean_grad`)."""
        solver = self._gradient_solver(solver)
        dev, md, rows = self._pack(update_caches=False)
        out = self._own(self._mean_grad_call(dev, md, rows, solver))
        return float(out["lnl"]), dict(zip(self.mean_gradient_labels, (float(v) for v in out["grad"])))

    def log_likelihood_mean_gradient_batch(self, P, return_info=False, solver=None):
        """:meth:`log_likelihood_mean_gradient` for B walkers (rows of ``P`` in :attr:`labels` order) in one batched device
        pass: ``(lnL (B,), grad (B, len(mean_gradient_labels)))``.  Walkers that fail get ``-inf`` and a NaN row, ``info`` their
        codes.  The model's own state is not modified.  ``solver``: as for :meth:`log_likelihood_mean_gradient`."""
        solver = self._gradient_solver(solver)
        P = np.atleast_2d(np.asarray(P, dtype=np.float64))
        dev, md, rows = self._pack(P, update_caches=False)
        out = self._mean_grad_call(dev, md, rows, solver)
        lnl = np.where(out["info"] == 0, out["lnl"], -np.inf)
        return (lnl, out["grad"], out["info"]) if return_info else (lnl, out["grad"])

    # ------------------------------------------------------------------ Fisher information in the mean-flux parameters
    def _fisher_call(self, dev, md, rows, solver):
        """The device call of the Fisher matrix in the columns of :meth:`_mean_gradient_columns` (and so with its refusals)."""
        return dev.fisher_mean(md, rows, self._mean_gradient_columns(dev, md), solver=solver)

    def fisher_information(self, solver=None):
        """The Fisher information of the mean-flux parameters at the current state and at fixed covariance, ``F_ij = fdot_i^T
        C^-1 fdot_j`` with ``fdot_j = d flux / d label_j``: a ``(p, p)`` array in :attr:`mean_gradient_labels` order, symmetric
        bit for bit.  This is the Gauss-Newton, fixed-covariance matrix: the term ``1/2 tr(C^-1 dC_i C^-1 dC_j)`` that a grid
        parameter has because the emulator's rows sit inside the covariance is left out; the block of the covariance
        hyper-parameters is :meth:`covariance_fisher_information` (the mean / covariance cross block of a Gaussian's Fisher matrix
        is zero).  Raises as
        :meth:`log_likelihood` does and refuses what :meth:`log_likelihood_mean_gradient` refuses; the model's state is not
        modified.  ``solver``: ``None`` / "dense" the dense factor, "banded" / "auto" one sweep of the band + Woodbury solver
        (:meth:`DeviceOrder.fisher_mean`)."""
        solver = self._gradient_solver(solver)
        dev, md, rows = self._pack(update_caches=False)
        return self._own(self._fisher_call(dev, md, rows, solver))["fisher"]

    def fisher_information_batch(self, P, return_info=False, solver=None):
        """:meth:`fisher_information` for B walkers (rows of ``P`` in :attr:`labels` order) in one batched device pass:
        ``(B, p, p)``, a NaN matrix for a walker that fails; with ``return_info`` ``(fisher, info)``.  The model's own state is
        not modified."""
        solver = self._gradient_solver(solver)
        P = np.atleast_2d(np.asarray(P, dtype=np.float64))
        dev, md, rows = self._pack(P, update_caches=False)
        out = self._fisher_call(dev, md, rows, solver)
        return (out["fisher"], out["info"]) if return_info else out["fisher"]

    # ------------------------------------------------------------------ Fisher information in the covariance hyper-parameters
    def _cov_fisher(self, out, md):
        """The rows and columns of :attr:`gradient_labels` of the device's matrices (the last two axes of ``out["fisher"]``)."""
        slots = self._gradient_slots(md)
        return out["fisher"][..., slots, :][..., :, slots]

    def covariance_fisher_information(self):
        """The Fisher information of the covariance hyper-parameters at the current state, ``F_ij = 1/2 tr(C^-1 dC_i C^-1
        dC_j)`` with ``dC_i = d C / d label_i``: a ``(q, q)`` array in :attr:`gradient_labels` order, symmetric bit for bit
        (sf_fisher_cov_batch).  The device differentiates in every slot; frozen labels drop their rows and columns.  In ``mu`` of
        a local kernel the derivative is the almost-everywhere one, as for :meth:`log_likelihood_gradient`.  Always the dense
        factor, whatever the model's ``solver`` is: the band of the inverse does not hold ``C^-1 dC_i C^-1``.  Raises
        ``ValueError`` if no covariance label is thawed, and as :meth:`log_likelihood` does; the model's state is not modified."""
        if not self.gradient_labels:
            raise ValueError("no thawed global_cov / local_cov parameter to take the Fisher information in")
        dev, md, rows = self._pack(update_caches=False)
        return self._cov_fisher(self._own(dev.fisher_cov(md, rows)), md)

    def covariance_fisher_information_batch(self, P, return_info=False):
        """:meth:`covariance_fisher_information` for B walkers (rows of ``P`` in :attr:`labels` order) in one batched device
        pass: ``(B, q, q)``, a NaN matrix for a walker that fails; with ``return_info`` ``(fisher, info)``.  The model's own state
        is not modified."""
        if not self.gradient_labels:
            raise ValueError("no thawed global_cov / local_cov parameter to take the Fisher information in")
        P = np.atleast_2d(np.asarray(P, dtype=np.float64))
        dev, md, rows = self._pack(P, update_caches=False)
        out = dev.fisher_cov(md, rows)
        fisher = self._cov_fisher(out, md)
        return (fisher, out["info"]) if return_info else fisher

    @property
    def fisher_labels(self):
        """tuple of str : the thawed labels in :attr:`labels` order without ``Rv``: the labels of
        ``parameter_covariance(include_covariance=True)``."""
        return tuple(key for key in self.labels if key != "Rv")

    def parameter_covariance(self, priors=None, solver=None, include_covariance=False):
        """The Laplace covariance of the labels of :attr:`mean_gradient_labels` at the current state (the point :meth:`train`
        found): the inverse of :meth:`fisher_information` plus, for every prior on one of these labels,
        ``-d^2 logpdf / d label^2`` by a central second difference with the step of the trainers' prior slopes,
        ``eps^(1/3) max(1, |x|)``.  The covariance hyper-parameters are held fixed; see :meth:`fisher_information` for what
        the matrix leaves out.  The inverse is formed in normalised form, ``D^-1 (D^-1 F D^-1)^-1 D^-1`` with ``D =
        sqrt(diag(F))``, by Cholesky; a matrix that is not positive definite (parameters the data do not separate) raises
        ``np.linalg.LinAlgError`` naming the labels (:func:`starfish_amd._map.laplace_covariance`).  ``priors`` are checked as
        :meth:`train` checks them.

        ``include_covariance=True``: the Laplace covariance of :attr:`fisher_labels`, the thawed covariance hyper-parameters
        included.  The assembled Fisher matrix has :meth:`fisher_information` (``solver``) in the mean-flux labels,
        :meth:`covariance_fisher_information` in the covariance labels and a zero cross block, and goes once through the same
        inversion, with priors on either kind of label; either block may be empty.  This is an approximation: the grid
        parameters and ``log_scale`` also sit inside ``C`` through the emulator term, and their ``1/2 tr(C^-1 dC_i C^-1 dC_j)``
        terms, with each other and with the hyper-parameters, are left out of both blocks and of the cross block."""
        priors = self._checked_priors(priors)
        if not include_covariance:
            labels = self.mean_gradient_labels
            terms = [(i, priors[key], float(self[key])) for i, key in enumerate(labels) if key in priors]
            return _map.laplace_covariance(self.fisher_information(solver=solver), labels, terms)
        labels = self.fisher_labels
        if not labels:
            raise ValueError("no thawed parameter to take the covariance of")
        F = np.zeros((len(labels), len(labels)))
        mean = [labels.index(key) for key in self.mean_gradient_labels]
        cov = [labels.index(key) for key in self.gradient_labels]
        if mean:
            F[np.ix_(mean, mean)] = self.fisher_information(solver=solver)
        if cov:
            F[np.ix_(cov, cov)] = self.covariance_fisher_information()
        terms = [(i, priors[key], float(self[key])) for i, key in enumerate(labels) if key in priors]
        return _map.laplace_covariance(F, labels, terms)

    def _scatter_combined(self, grad, md, out, columns):
        """A combined device result -- the mean ``columns`` in request order (none: ``[]``), then, where covariance labels are
        thawed, the covariance slots -- into the :attr:`labels`-ordered ``grad``; returns ``(lnl, info)`` with ``-inf`` for the
        walkers that failed."""
        labels, ncols = self.labels, len(columns)
        if columns:
            grad[:, [labels.index(key) for key in self.mean_gradient_labels]] = out["grad"][:, :ncols]
        if self.gradient_labels:
            grad[:, [labels.index(key) for key in self.gradient_labels]] = out["grad"][:, [ncols + s for s in self._gradient_slots(md)]]
        return np.where(out["info"] == 0, out["lnl"], -np.inf), out["info"]

    def log_likelihood_full_gradient_batch(self, P, return_info=False, one_pass=False, solver=None, covariance_solver=None):
        """``(lnL (B,), grad (B, len(labels)))``: the gradient in every thawed label, columns in :attr:`labels` order -- the mean
        call's columns and, where covariance labels are thawed, :meth:`log_likelihood_gradient_batch`'s (two device calls).  A
        thawed ``Rv`` gets a zero column: it is never passed on.

        ``one_pass=True``: both parts from ONE factorisation per walker (sf_loglike_multi_grad_batch_md with one segment)
        instead of one per call; the values agree with the default's to rounding, not bit for bit.

        ``solver``: as for :meth:`log_likelihood_mean_gradient`, for the mean columns.  ``covariance_solver``: as for
        :meth:`log_likelihood_gradient`, for the covariance columns (and with them ``lnL``, where covariance labels are
        thawed); ``None`` is the dense factor whatever ``solver`` is.  Where both are "banded" or both "auto" and both kinds of
        label are thawed, everything comes from ONE device call on the band solver (sf_loglike_banded_grad_batch), with the
        bits of the two separate calls.  ``one_pass=True`` is the dense factor's: with another solver it raises ``ValueError``."""
        solver = self._gradient_solver(solver)
        covariance_solver = self._gradient_solver(covariance_solver)
        if one_pass and (solver != "dense" or covariance_solver != "dense"):
            raise ValueError('one_pass=True shares ONE dense factorisation: it takes solver / covariance_solver None or "dense" only')
        P = np.atleast_2d(np.asarray(P, dtype=np.float64))
        labels = self.labels
        grad = np.zeros((P.shape[0], len(labels)))
        lnl = info = None
        if one_pass:
            mean, cov = self.mean_gradient_labels, self.gradient_labels
            if not mean and not cov:
                raise ValueError("no thawed parameter to differentiate in")
            dev, md, rows = self._pack(P, update_caches=False)
            columns = self._mean_gradient_columns(dev, md) if mean else []
            lnl, info = self._scatter_combined(grad, md, M.loglike_multi_grad([dev], [md], [rows], [(columns, bool(cov))])[0], columns)
            return (lnl, grad, info) if return_info else (lnl, grad)
        if solver == covariance_solver != "dense" and self.mean_gradient_labels and self.gradient_labels:
            dev, md, rows = self._pack(P, update_caches=False)
            columns = self._mean_gradient_columns(dev, md)
            lnl, info = self._scatter_combined(grad, md, dev.loglike_banded_grad(md, rows, columns, True, solver=solver), columns)
            return (lnl, grad, info) if return_info else (lnl, grad)
        if self.mean_gradient_labels:
            lnl, g, info = self.log_likelihood_mean_gradient_batch(P, return_info=True, solver=solver)
            grad[:, [labels.index(key) for key in self.mean_gradient_labels]] = g
        if self.gradient_labels:
            lnl, g, info = self.log_likelihood_gradient_batch(P, return_info=True, solver=covariance_solver)
            grad[:, [labels.index(key) for key in self.gradient_labels]] = g
        if lnl is None:
            raise ValueError("no thawed parameter to differentiate in")
        return (lnl, grad, info) if return_info else (lnl, grad)

    def _train_gradient(self, priors, kwargs, solver=None, covariance_solver=None):
        """The ``gradient=True`` search of :meth:`train`; ``solver``: of the mean columns (``gradient_solver``),
        ``covariance_solver``: of the covariance columns."""
        solver, covariance_solver = self._gradient_solver(solver), self._gradient_solver(covariance_solver)

        def evaluate(x):
            self.set_param_vector(x)
            lnl, grad, info = self.log_likelihood_full_gradient_batch(x[None, :], return_info=True, solver=solver,
                                                                       covariance_solver=covariance_solver)
            self._raise_for_info(info[0])
            return lnl[0], grad[0]

        soln = _map.minimize_lbfgsb(evaluate, self.get_param_vector().astype(np.float64),
                                    *self._prior_split(priors, self.labels), kwargs, finite_for="SpectrumModel.train")
        if soln.success or soln.status == 1:  # (1: the iteration / evaluation limit; soln.x is the best point so far)
            self.set_param_vector(soln.x)
        return soln
