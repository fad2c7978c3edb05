"""The factor-applied diagnostics of :class:`SpectrumModel`: the Cholesky factor of the covariance applied to right-hand
sides, the residual split by covariance component, the per-pixel leave-one-out predictive.  Not likelihood evaluations: none
of them touches residuals, _lnprob, _log_scale or the covariance caches.

``solver`` (cho_solve, apply_factor_batch with "Cinv", residual_components, pointwise and their batch forms): None is the dense
factor whatever the model's own ``solver`` is, so that every call keeps its bits; "banded" / "auto" take the band + Woodbury solver
as the gradient methods do (:meth:`DeviceOrder.diagnose_banded`)."""
import numpy as np

from .. import _device as D


class Diagnostics:
    # ------------------------------------------------------------------ the Cholesky factor of the covariance, applied
    def _rhs_block(self, rhs, what="rhs"):
        """``rhs`` as a (k, n) block, and whether it came as one vector."""
        r = np.asarray(rhs, dtype=np.float64)
        if r.ndim not in (1, 2) or r.shape[-1] != len(self.data.wave):
            raise ValueError(f"{what} of shape {r.shape}: expected ({len(self.data.wave)},) or (k, {len(self.data.wave)})")
        return np.atleast_2d(r), r.ndim == 1

    def _diagnose(self, call, P, rhs, *args, **kwargs):
        """``DeviceOrder.<call>`` on the rows of ``P`` (None: the model's own state, one walker) and the right-hand sides
        ``rhs``, with whatever else the call takes: its result, the model descriptor, ``rhs`` as handed to the device and
        whether every walker has one vector.  No cache is updated."""
        if rhs is None:
            single = True
        else:
            rhs, single = self._rhs_block(rhs) if P is None else self._batch_rhs(P, rhs)
        solver = self._gradient_solver(kwargs.pop("solver", None))
        if solver != "dense":  # ("dense" is the call as it always was)
            kwargs["solver"] = solver
        dev, md, rows = self._pack(P, update_caches=False)
        return getattr(dev, call)(md, rows, *args, rhs=rhs, **kwargs), md, rhs, single

    def _own(self, out):
        """The first walker of a device result, or what :meth:`log_likelihood` raises for its status."""
        self._raise_for_info(out["info"][0])
        return {key: v[0] for key, v in out.items()}

    def _apply_factor(self, op, rhs, want_flux=False, solver=None):
        """``op`` of :meth:`apply_factor_batch` for the current parameters; raises as :meth:`log_likelihood` does."""
        out, _, _, single = self._diagnose("apply", None, rhs, op, want_flux=want_flux, solver=solver)
        out = self._own(out)
        return (out["out"][0] if single else out["out"]), (out["flux"] if want_flux else None)

    def cho_solve(self, rhs=None, solver=None):
        """``C^-1 rhs`` for the covariance of the current parameters, jitter included (the reference's
        ``cho_solve(factor, R)``, spectrum_model.py:404), solved on the device with the factor the likelihood uses.
        ``rhs``: (n,) or (k, n); None = the current residual ``flux - data.flux``.  ``solver``: None or "dense" -- the
        dense factor; "banded" / "auto" -- the band + Woodbury solver, as in :meth:`log_likelihood_gradient`."""
        return self._apply_factor("Cinv", rhs, solver=solver)[0]

    def whiten(self, rhs=None):
        """``L^-1 rhs`` (C = L L^T): iid N(0, 1) if ``rhs`` is noise drawn from C.  None = the current residual.  Always the
        dense factor: the band + Woodbury solver factorises Bd and the capacitance matrix, not C, so it has no triangular L
        with C = L L^T to apply."""
        return self._apply_factor("Linv", rhs)[0]

    def draw(self, size=None, rng=None, z=None):
        """Noise realisations ``flux + L z`` of the current model.  Pass standard-normal ``z`` of shape (n,) or (k, n), or
        ``size`` (None: one draw of shape (n,); k: (k, n)) and ``rng`` (a ``numpy.random.Generator`` or a seed).  Always the
        dense factor, for the reason :meth:`whiten` gives."""
        n = len(self.data.wave)
        if z is None:
            gen = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
            z = gen.standard_normal(n if size is None else (int(size), n))
        elif size is not None:
            raise ValueError("pass either z or size, not both")
        lz, flux = self._apply_factor("L", z, want_flux=True)
        return flux + lz

    def apply_factor_batch(self, P, op, rhs=None, return_info=False, solver=None):
        """The factor of B walkers' covariance matrices (rows of ``P`` in :attr:`labels` order) applied in one batched
        device pass: ``op`` "L" (L rhs), "Linv" (L^-1 rhs), "LinvT" (L^-T rhs) or "Cinv" (C^-1 rhs).  ``rhs``: None (each
        walker's own residual), (n,) / (k, n) shared by all walkers, or (B, k, n).  Returns (B, k, n) -- (B, n) for None
        or (n,) --; walkers that fail (outside the emulator grid, covariance not positive definite, ...) get NaN rows,
        ``info`` the codes of :meth:`log_likelihood_batch`.  The model's own state is not modified.  ``solver``: as for
        :meth:`cho_solve`, with "Cinv" only: another ``op`` with the band solver is a ``ValueError``."""
        if op not in D.APPLY_OPS:
            raise ValueError(f"op must be one of {sorted(D.APPLY_OPS)}")
        if op != "Cinv" and self._gradient_solver(solver) != "dense":
            raise ValueError(f'op {op!r} needs the dense factor: solver={solver!r} takes "Cinv" only')
        out, _, _, single = self._diagnose("apply", np.atleast_2d(np.asarray(P, dtype=np.float64)), rhs, op, solver=solver)
        res = out["out"][:, 0] if single else out["out"]
        return (res, out["info"]) if return_info else res

    def _batch_rhs(self, P, rhs):
        """``rhs`` of the batched diagnostics: (n,) / (k, n) shared by the walkers, or (B, k, n); and whether every walker
        has one vector."""
        r = np.asarray(rhs, dtype=np.float64)
        if r.ndim == 3:
            if r.shape[0] != P.shape[0] or r.shape[-1] != len(self.data.wave):
                raise ValueError(f"rhs of shape {r.shape}: expected ({P.shape[0]}, k, {len(self.data.wave)})")
            return r, False
        return self._rhs_block(r)

    # ------------------------------------------------------------------ the residual split by covariance component
    # C = Y^T Y (emulator) + diag(sigma^2 + 1e-10) (noise) + K_global + sum_j K_local,j: the conditional mean of each term
    # given the residual is K_k alpha with alpha = C^-1 r; the means add up to r.  Diagnostics like the ones above.
    @staticmethod
    def _component_dict(comp, alpha, has_global, n_local, single):
        """The component axis of :meth:`DeviceOrder.decompose` as a dict: ``comp`` (..., 3 + n_local, k, n) and ``alpha``
        (..., k, n) -> emulator, noise, global (with ``has_global``), local (..., n_local, k, n) (with local kernels) and
        alpha; the k axis is dropped for ``single``."""
        comp, alpha = np.asarray(comp), np.asarray(alpha)
        if comp.ndim < 3 or comp.shape[-3] != 3 + n_local or alpha.shape != comp.shape[:-3] + comp.shape[-2:]:
            raise ValueError(f"components of shape {comp.shape} and alpha of shape {alpha.shape} do not belong to a model "
                             f"with {n_local} local kernel(s)")
        pick = (lambda a: a[..., 0, :]) if single else (lambda a: a)
        out = {"emulator": pick(comp[..., 0, :, :]), "noise": pick(comp[..., 1, :, :])}
        if has_global:
            out["global"] = pick(comp[..., 2, :, :])
        if n_local:
            out["local"] = pick(comp[..., 3:, :, :])
        out["alpha"] = pick(alpha)
        return out

    def residual_components(self, rhs=None, solver=None):
        """The conditional mean of every covariance component given ``rhs`` (None: the current residual ``flux -
        data.flux``; (n,) or (k, n)): dict with "emulator", "noise", "global" (models with ``global_cov``), "local"
        (models with ``local_cov``: one row per kernel, in the order of ``self["local_cov"]``) and "alpha" = ``C^-1 rhs``
        (:meth:`cho_solve`).  The components add up to ``rhs``.  Raises as :meth:`log_likelihood` does.  ``solver``: as for
        :meth:`cho_solve`."""
        out, md, _, single = self._diagnose("decompose", None, rhs, solver=solver)
        out = self._own(out)
        return self._component_dict(out["comp"], out["alpha"], bool(md.has_global), int(md.n_local), single)

    def residual_components_batch(self, P, rhs=None, return_info=False, solver=None):
        """:meth:`residual_components` for B walkers (rows of ``P`` in :attr:`labels` order) in one batched device pass:
        the same keys with a leading B axis.  ``rhs`` as for :meth:`apply_factor_batch`; walkers that fail get NaN rows,
        ``info`` their codes.  The model's own state is not modified.  ``solver``: as for :meth:`cho_solve`."""
        out, md, _, single = self._diagnose("decompose", np.atleast_2d(np.asarray(P, dtype=np.float64)), rhs, solver=solver)
        res = self._component_dict(out["comp"], out["alpha"], bool(md.has_global), int(md.n_local), single)
        return (res, out["info"]) if return_info else res

    # ------------------------------------------------------------------ per-pixel leave-one-out diagnostics
    # Pixel i predicted from all the others under the fitted covariance (Rasmussen & Williams, Gaussian Processes for
    # Machine Learning, 5.4.2): with alpha = C^-1 r and d = diag(C^-1), mean r_i - alpha_i / d_i and variance 1 / d_i.
    @staticmethod
    def _pointwise_dict(rhs, alpha, cinv_diag, cov_diag, single):
        """The results of :meth:`DeviceOrder.pointwise` as the dict of :meth:`pointwise`: ``rhs`` and ``alpha`` (..., k, n),
        ``cinv_diag`` and ``cov_diag`` (..., n); the k axis is dropped for ``single``."""
        rhs, alpha = np.asarray(rhs, dtype=np.float64), np.asarray(alpha, dtype=np.float64)
        cinv_diag, cov_diag = np.asarray(cinv_diag, dtype=np.float64), np.asarray(cov_diag, dtype=np.float64)
        if alpha.ndim < 2 or cinv_diag.shape != alpha.shape[:-2] + alpha.shape[-1:] or cov_diag.shape != cinv_diag.shape:
            raise ValueError(f"alpha of shape {alpha.shape}, cinv_diag of shape {cinv_diag.shape} and cov_diag of shape "
                             f"{cov_diag.shape} do not belong together")
        rhs = np.broadcast_to(rhs, alpha.shape)
        d = cinv_diag[..., None, :]
        z = alpha / np.sqrt(d)
        pick = (lambda a: a[..., 0, :]) if single else (lambda a: a)
        return {
            "alpha": pick(alpha),
            "marginal_std": np.sqrt(cov_diag),
            "loo_mean": pick(rhs - alpha / d),
            "loo_std": 1.0 / np.sqrt(cinv_diag),
            "z": pick(z),
            "log_density": pick(-0.5 * np.log(2.0 * np.pi / d) - 0.5 * z * z),
        }

    def pointwise(self, rhs=None, solver=None):
        """Every pixel of ``rhs`` (None: the current residual ``flux - data.flux``; (n,) or (k, n)) judged against the
        prediction from all the OTHER pixels under the covariance of the current parameters: dict with "alpha" = ``C^-1
        rhs`` (:meth:`cho_solve`), "marginal_std" = ``sqrt(diag(C))`` (jitter included; the band the reference's plot
        shades), "loo_mean" = ``rhs - alpha / d`` and "loo_std" = ``1 / sqrt(d)`` with ``d = diag(C^-1)``, the
        standardised residual "z" = ``alpha / sqrt(d)`` and the per-pixel "log_density" = ``-log(2 pi / d) / 2 - z^2 / 2``,
        whose sum is the leave-one-out pseudo-likelihood.  "marginal_std" and "loo_std" are (n,) whatever ``rhs`` is.
        Raises as :meth:`log_likelihood` does.  ``solver``: as for :meth:`cho_solve`."""
        out, _, rhs, single = self._diagnose("pointwise", None, rhs, want_flux=rhs is None, solver=solver)
        out = self._own(out)
        if rhs is None:
            rhs = (out["flux"] - self.data.flux)[None, :]
        return self._pointwise_dict(rhs, out["alpha"], out["cinv_diag"], out["cov_diag"], single)

    def pointwise_batch(self, P, rhs=None, return_info=False, solver=None):
        """:meth:`pointwise` for B walkers (rows of ``P`` in :attr:`labels` order) in one batched device pass: the same
        keys with a leading B axis.  ``rhs`` as for :meth:`apply_factor_batch`; walkers that fail get NaN rows, ``info``
        their codes.  The model's own state is not modified.  ``solver``: as for :meth:`cho_solve`."""
        out, _, rhs, single = self._diagnose("pointwise", np.atleast_2d(np.asarray(P, dtype=np.float64)), rhs,
                                             want_flux=rhs is None, solver=solver)
        if rhs is None:
            rhs = (out["flux"] - self.data.flux)[:, None, :]
        res = self._pointwise_dict(rhs, out["alpha"], out["cinv_diag"], out["cov_diag"], single)
        return (res, out["info"]) if return_info else res
