"""The factor-applied diagnostics of :class:`SpectrumModel`: the Cholesky factor of the covariance applied to right-hand
sides, the residual split by covariance component, the per-pixel leave-one-out predictive, the score scan for new local
kernels.  Not likelihood evaluations: none of them touches residuals, _lnprob, _log_scale or the covariance caches.

``solver`` (cho_solve, apply_factor_batch with "Cinv", residual_components, pointwise and their batch forms): None is the dense
factor whatever the model's own ``solver`` is, so that every call keeps its bits; "banded" / "auto" take the band + Woodbury solver
as the gradient methods do (:meth:`DeviceOrder.diagnose_banded`)."""
import numpy as np

from .. import _device as D

DEFAULT_SCAN_SIGMAS = (8.0, 15.0, 30.0)  # km/s


def pick_local_kernels(z, amp, mus, sigmas, threshold=4.0, buffer=None, max_kernels=None):
    """The peak picking of :meth:`Diagnostics.propose_local_kernels` as a pure function.  ``z`` and ``amp``: (len(sigmas),
    len(mus)) score statistics and Newton amplitudes; ``mus`` in the units of the wavelengths, ``sigmas`` in km/s.

    Per centre the width with the largest ``z`` (the first of equal ones; NaN entries do not count, a centre with nothing but NaN
    is left out).  Centres with ``z > threshold`` and a positive amplitude are walked from the largest ``z`` down (equal ``z``:
    the smaller ``mu`` first); one that lies within ``buffer`` of a kept centre is dropped -- ``buffer`` None: within the kept
    kernel's own reach ``4 sigma mu / c``.  At most ``max_kernels`` are kept (None: no limit).  Returns the list, sorted by
    ``mu``, of ``{"mu", "log_amp", "log_sigma"}``."""
    z, amp = np.atleast_2d(np.asarray(z, dtype=np.float64)), np.atleast_2d(np.asarray(amp, dtype=np.float64))
    mus, sigmas = np.atleast_1d(np.asarray(mus, dtype=np.float64)), np.atleast_1d(np.asarray(sigmas, dtype=np.float64))
    if z.shape != (len(sigmas), len(mus)) or amp.shape != z.shape:
        raise ValueError(f"z of shape {z.shape} and amp of shape {amp.shape}: expected ({len(sigmas)}, {len(mus)})")
    if max_kernels is not None and max_kernels <= 0:
        return []
    cols = np.nonzero(~np.isnan(z).all(axis=0))[0]
    best = np.argmax(np.where(np.isnan(z[:, cols]), -np.inf, z[:, cols]), axis=0)
    zbest, abest = z[best, cols], amp[best, cols]
    ok = (zbest > threshold) & (abest > 0) & np.isfinite(abest)
    cols, best, zbest, abest = cols[ok], best[ok], zbest[ok], abest[ok]
    kept = []
    for i in np.lexsort((mus[cols], -zbest)):
        mu, sg = float(mus[cols[i]]), float(sigmas[best[i]])
        if any(abs(mu - k["mu"]) <= (k["reach"] if buffer is None else buffer) for k in kept):
            continue
        kept.append({"mu": mu, "log_amp": float(np.log(abest[i])), "log_sigma": float(np.log(sg)), "reach": 4 * sg * mu / D.C_KMS})
        if max_kernels is not None and len(kept) >= max_kernels:
            break
    return [{key: k[key] for key in ("mu", "log_amp", "log_sigma")} for k in sorted(kept, key=lambda k: k["mu"])]


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

    # ------------------------------------------------------------------ where does a new local kernel belong?
    # The score (Lagrange-multiplier) test for adding a local kernel of centre mu and width sigma at amplitude A = 0 to the
    # covariance as it stands: with k the matrix the kernel adds at amplitude 1, alpha = C^-1 r and W = C^-1,
    # U = d lnL / dA = 1/2 (alpha^T k alpha - tr(W k)), its information I = 1/2 tr(W k W k), z = U / sqrt(I), A = U / I.
    def _scan_candidates(self, mus, sigmas, wl_range, banded_limit=None):
        """The centres and widths of a scan, checked on the host: (mus, sigmas, (len(sigmas) * len(mus), 2) candidate rows,
        width-major).  ``banded_limit``: under ``solver="banded"`` the widest patch the band solver serves."""
        wave = np.asarray(self.data.wave, dtype=np.float64)
        mus = wave.copy() if mus is None else np.atleast_1d(np.asarray(mus, dtype=np.float64)).copy()
        if wl_range is not None:
            lo, hi = wl_range
            mus = mus[(mus >= lo) & (mus <= hi)]
        sigmas = np.atleast_1d(np.asarray(sigmas, dtype=np.float64))
        if mus.ndim != 1 or sigmas.ndim != 1 or not mus.size or not sigmas.size:
            raise ValueError("the scan needs at least one centre and one width")
        if not (np.isfinite(mus).all() and (mus > 0).all() and np.isfinite(sigmas).all() and (sigmas > 0).all()):
            raise ValueError("the centres (wavelengths) and the widths (km/s) of the scan must be positive and finite")
        cand = np.stack([np.tile(mus, len(sigmas)), np.repeat(sigmas, len(mus))], axis=1)
        lo, hi = D.local_scan_patches(wave, cand)
        wide = np.nonzero(hi - lo + 1 > D.LOCAL_SCAN_MAX_PATCH)[0]
        if wide.size:
            q = int(wide[0])
            raise ValueError(f"candidate mu={float(cand[q, 0])!r}, sigma={float(cand[q, 1])!r} km/s reaches {int(hi[q] - lo[q] + 1)} pixels: the "
                             f"device scans patches of at most {D.LOCAL_SCAN_MAX_PATCH} pixels")
        if banded_limit is not None:
            wide = np.nonzero(hi - lo + 1 > banded_limit)[0]
            if wide.size:
                q = int(wide[0])
                raise ValueError(f"candidate mu={float(cand[q, 0])!r}, sigma={float(cand[q, 1])!r} km/s reaches {int(hi[q] - lo[q] + 1)} pixels: the "
                                 f"band solver scans patches of at most {int(banded_limit)} pixels (solver=\"auto\" takes the dense factor "
                                 "for such a scan)")
        return mus, sigmas, cand

    def _local_scan(self, P, mus, sigmas, wl_range, solver=None):
        """The scan of the rows of ``P`` (None: the model's own state): the result dict with a leading walker axis, the status,
        the centres and the widths.  No cache is updated.  ``solver``: None / "dense" is the call as it always was; "banded" /
        "auto" are handed to :meth:`DeviceOrder.local_scan`, "banded" after the candidates were held to its patch limit."""
        solver = self._gradient_solver(solver)
        limit = None
        if solver == "banded":  # (a size query of the order's context; nothing is enqueued)
            dev, md, _ = self._pack(P, update_caches=False)
            limit = dev.local_scan_banded_max_patch(md)
        mus, sigmas, cand = self._scan_candidates(mus, DEFAULT_SCAN_SIGMAS if sigmas is None else sigmas, wl_range, limit)
        dev, md, rows = self._pack(P, update_caches=False)
        kw = {} if solver == "dense" else {"solver": solver}
        step = 65535  # (candidates per device call)
        parts = [dev.local_scan(md, rows, cand[q:q + step], **kw) for q in range(0, len(cand), step)]
        shape = (rows.shape[0], len(sigmas), len(mus))
        quad, trace, fisher = (np.concatenate([p[key] for p in parts], axis=1).reshape(shape) for key in ("quad", "trace", "fisher"))
        score = 0.5 * (quad - trace)
        with np.errstate(divide="ignore", invalid="ignore"):
            z = np.where(fisher == 0, np.nan, score / np.sqrt(fisher))
            amp = np.where(fisher == 0, np.nan, score / fisher)
        res = {"score": score, "information": fisher, "z": z, "amp": amp, "quad": quad, "trace": trace}
        return res, parts[0]["info"], mus, sigmas

    def local_kernel_scan(self, mus=None, sigmas=None, wl_range=None, solver=None):
        """The score test for one more local kernel, for every centre in ``mus`` (None: every pixel's wavelength; ``wl_range`` =
        (lo, hi) keeps the centres inside it) and every width in ``sigmas`` (km/s; None: 8, 15, 30), at the current parameters
        and with every kernel the model already has in the covariance (sf_local_scan_batch): dict of arrays of shape
        (len(sigmas), len(mus)) with "score" = ``d lnL / dA`` at amplitude A = 0, "information" = its Fisher information, "z" =
        ``score / sqrt(information)``, "amp" = ``score / information`` (one Newton step in A), and the pieces "quad" = ``alpha^T k
        alpha`` and "trace" = ``tr(C^-1 k)``.  "z" and "amp" are NaN where the information is 0 (no pixel within 4 sigma of the
        centre).  A candidate that reaches more pixels than the device scans is a ``ValueError`` before any device call.  Raises
        as :meth:`log_likelihood` does; the model's state is not modified.

        ``solver``: None or "dense" -- the dense factor, whatever the model's own ``solver`` is; "banded" -- the band + Woodbury
        solver and its selected inversion (sf_local_scan_banded_batch; values agree with the dense scan to rounding), which serves
        patches of at most :meth:`DeviceOrder.local_scan_banded_max_patch` pixels (145 for up to 15 emulator components): a wider
        candidate is a ``ValueError`` before any device call; "auto" -- the band solver where it serves every candidate and the
        walker's covariance fits its window, the dense factor otherwise."""
        res, info, _, _ = self._local_scan(None, mus, sigmas, wl_range, solver)
        self._raise_for_info(info[0])
        return {key: v[0] for key, v in res.items()}

    def local_kernel_scan_batch(self, P, mus=None, sigmas=None, wl_range=None, return_info=False, solver=None):
        """:meth:`local_kernel_scan` for B walkers (rows of ``P`` in :attr:`labels` order) in one batched device pass: the same
        keys with a leading B axis.  Walkers that fail get NaN rows, ``info`` their codes (those of
        :meth:`log_likelihood_batch`).  The model's own state is not modified.  ``solver``: as for :meth:`local_kernel_scan`."""
        res, info, _, _ = self._local_scan(np.atleast_2d(np.asarray(P, dtype=np.float64)), mus, sigmas, wl_range, solver)
        return (res, info) if return_info else res

    def propose_local_kernels(self, threshold=4.0, buffer=None, max_kernels=None, sigmas=None, mus=None, wl_range=None, P=None,
                              solver=None):
        """Where the residual asks for local kernels: :meth:`local_kernel_scan` (with ``P``: :meth:`local_kernel_scan_batch`, ``z``
        and ``amp`` averaged over the walkers that evaluate), then per centre the width with the largest ``z``, the centres with
        ``z > threshold`` walked from the largest ``z`` down, a centre within ``buffer`` (the units of the wavelengths; None: the
        kept kernel's own reach of 4 sigma) of a kept one dropped, at most ``max_kernels`` kept (None: as many as the model can
        still take).  Returns the list, sorted by ``mu``, of ``{"mu", "log_amp", "log_sigma"}`` with ``log_amp = log(amp)`` of the
        Newton step: what ``model["local_cov"] = [*kernels_it_has, *model.propose_local_kernels()]`` takes, to be refined by
        :meth:`train_covariance`.  The model is never changed.  ``solver``: as for :meth:`local_kernel_scan`.

        ``z`` is a score statistic at FIXED remaining parameters, and one-sided: the amplitude of a kernel cannot be negative,
        so only an excess of correlated residual power (``z > 0``) proposes one; under the null ``z`` is about standard normal
        per candidate, and the largest of a whole scan of a few thousand correlated candidates reaches 3 by chance.  Candidates
        are tested one at a time: two proposals may explain the same feature where the buffer lets them.  The reference's
        ``find_residual_peaks`` / ``optimize_residual_peaks`` instead sigma-clip the averaged residuals and fit each peak's
        kernel by Nelder-Mead on the full likelihood; here the covariance that is already fitted (global kernel, emulator,
        existing local kernels) is accounted for exactly, every pixel and width is tested, and nothing is refitted."""
        if P is None:
            res, info, mus, sigmas = self._local_scan(None, mus, sigmas, wl_range, solver)
            self._raise_for_info(info[0])
            z, amp = res["z"][0], res["amp"][0]
        else:
            res, info, mus, sigmas = self._local_scan(np.atleast_2d(np.asarray(P, dtype=np.float64)), mus, sigmas, wl_range, solver)
            good = info == 0
            if not good.any():
                raise ValueError("no walker of P evaluates: nothing to average")
            z, amp = res["z"][good].mean(axis=0), res["amp"][good].mean(axis=0)
        if max_kernels is None:
            max_kernels = D.MAX_LOCAL - len(self._local_kernels())
        return pick_local_kernels(z, amp, mus, sigmas, threshold, buffer, max_kernels)
