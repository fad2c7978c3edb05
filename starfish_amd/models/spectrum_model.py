"""
``SpectrumModel`` -- the single-order forward model and Gaussian log-likelihood, with the reference's
Python surface (reference: Starfish/models/spectrum_model.py) so an existing emcee / scipy loop runs
unchanged, plus ``log_likelihood_batch`` which evaluates a whole block of walkers in one launch
sequence on the MI355X.

All numerics (transform chain, emulator query, fused covariance fill, batched Cholesky, solve) run in
the HIP kernels behind ``include/starfish_amd.h``; this file only keeps the parameter book-keeping
(FlatterDict store, labels, freeze / thaw, caches) and packs parameter rows for the C-ABI.
"""
import logging
import zlib
from collections import deque

import numpy as np

from .. import _device as D
from .._flatdict import FlatterDict
from ..emulator import Emulator
from ..spectrum import Spectrum
from ..transforms import resample
from ..utils import calculate_dv, create_log_lam_grid


try:  # content hash of the observation arrays (checked on every evaluation): xxh3 is ~20x faster than crc32
    from xxhash import xxh3_64_intdigest as _hash64
except ImportError:  # pragma: no cover
    _hash64 = zlib.crc32


def _digest(a):
    return _hash64(np.ascontiguousarray(a))


class SpectrumModel:
    """
    A single-order spectrum model (Starfish/models/spectrum_model.py:26-181).

    Parameters
    ----------
    emulator : Emulator or str
    data : Spectrum or str
        exactly one order (``ValueError`` otherwise, spectrum_model.py:141-144)
    grid_params : array-like
        values for ``emulator.param_names``
    max_deque_len, norm, name : as in the reference
    device : int, optional
        HIP device index holding this order's buffers (default: current device)
    **params :
        ``vz, vsini, Av, Rv, log_scale, global_cov={log_amp, log_ls},
        local_cov=[{mu, log_amp, log_sigma}, ...], cheb=[c1, c2, ...]``
    """

    _PARAMS = ["vz", "vsini", "Av", "Rv", "log_scale", "global_cov", "local_cov", "cheb"]
    _GLOBAL_PARAMS = ["log_amp", "log_ls"]
    _LOCAL_PARAMS = ["mu", "log_amp", "log_sigma"]

    def __init__(self, emulator, data, grid_params, max_deque_len=100, norm=False, name="SpectrumModel",
                 device=None, solver="dense", emulator_cov="code", **params):
        if isinstance(emulator, str):
            emulator = Emulator.load(emulator)
        if isinstance(data, str):
            data = Spectrum.load(data)
        if len(data) > 1:
            raise ValueError("Multiple orders detected in data, please use EchelleModel")

        self.emulator = emulator
        self.data_name = data.name
        self.data = data[0]
        self._device_index = device
        #: "dense" = the reference's algorithm (batched N x N Cholesky); "auto" = band + rank-m Woodbury
        #: solve whenever the covariance support fits the device window (same value to rounding, ~20x
        #: faster at N = 4096), dense otherwise; "banded" = structured solve only (info -4 if too wide)
        if solver not in ("dense", "banded", "auto"):
            raise ValueError("solver must be 'dense', 'banded' or 'auto'")
        self.solver = solver
        #: form of the emulator term of the covariance.  "code" (default, the parity target): X^T Sigma_w^-1 X, what the
        #: reference COMPUTES (spectrum_model.py:334-335: cho_solve of the weight covariance); "paper": X^T Sigma_w X, the
        #: form printed in the reference's docs (docs/api/emulator.rst:105) and in Czekala et al. (2015).
        if emulator_cov not in ("code", "paper"):
            raise ValueError("emulator_cov must be 'code' or 'paper'")
        self.emulator_cov = emulator_cov

        dv = calculate_dv(self.data.wave)
        self.min_dv_wave = create_log_lam_grid(dv, self.emulator.wl.min(), self.emulator.wl.max())["wl"]
        self._bulk_fluxes = None  # resampled lazily on the device (spectrum_model.py:154-156)
        self._dev = None
        self._dev_v11 = None
        self._dev_data = None

        self.residuals = deque(maxlen=max_deque_len)

        # cheb is stored as {"1": c1, "2": c2, ...}; re-inserting moves it behind the other kwargs
        if "cheb" in params:
            chebs = params.pop("cheb")
            params["cheb"] = {str(i): c for i, c in enumerate(chebs, start=1)}
        self.params = FlatterDict(params)
        self.frozen = []
        self.name = name
        self.norm = norm

        self.n_grid_params = len(grid_params)
        self.grid_params = grid_params

        self._lnprob = None
        self._glob_snapshot = None  # hyper-parameters the cached global kernel was built with
        self._loc_snapshot = None
        self._log_scale = params.get("log_scale", None)
        self.last_info = None

        self.log = logging.getLogger(self.__class__.__name__)

    # ------------------------------------------------------------------ lazily built device state
    @property
    def bulk_fluxes(self):
        """Emulator bulk fluxes resampled onto ``min_dv_wave`` (spectrum_model.py:154-156)."""
        if self._bulk_fluxes is None:
            self._bulk_fluxes = resample(self.emulator.wl, self.emulator.bulk_fluxes, self.min_dv_wave)
        return self._bulk_fluxes

    def _device(self):
        emu = self.emulator
        # the observation lives in HBM; the reference reads self.data on every evaluation
        # (spectrum_model.py:365-377), so a replaced or edited flux / sigma must reach the device copy
        d = self.data
        key = tuple(_digest(a) for a in (d.wave, d.flux, d.sigma))
        stale = self._dev is None or self._dev_v11 is not emu.v11 or key != self._dev_data
        if stale:
            if self._dev_data is not None and key[0] != self._dev_data[0]:
                # a new wavelength grid: what the constructor derived from it (spectrum_model.py:150-156) follows
                dv = calculate_dv(d.wave)
                self.min_dv_wave = create_log_lam_grid(dv, emu.wl.min(), emu.wl.max())["wl"]
                self._bulk_fluxes = None
            self._dev_data = key
            self._dev = D.DeviceOrder(
                self.data.wave, self.data.flux, self.data.sigma, self.min_dv_wave, self.bulk_fluxes,
                emu.grid_points, emu.variances, emu.lengthscales, emu.v11, emu.w_hat,
                device=self._device_index, emu_factor=emu.v11_factor(),
            )
            self._dev_v11 = emu.v11
        return self._dev

    # ------------------------------------------------------------------ covariance caches
    # The reference caches the N x N kernel matrices while their group is frozen
    # (spectrum_model.py:341-363).  Here the kernels are re-evaluated inside the fused fill, so the
    # cache keeps the hyper-parameters the matrix WOULD have been built with -- same observable
    # behaviour (a frozen group keeps using the values seen when the cache was filled).
    @property
    def _glob_cov(self):
        if self._glob_snapshot is None:
            return None
        from .kernels import global_covariance_matrix

        la, ll = self._glob_snapshot
        return global_covariance_matrix(self.data.wave, np.exp(la), np.exp(ll))

    @_glob_cov.setter
    def _glob_cov(self, value):
        if value is not None:
            raise AttributeError("_glob_cov can only be reset to None")
        self._glob_snapshot = None

    @property
    def _loc_cov(self):
        if self._loc_snapshot is None:
            return None
        from .kernels import local_covariance_matrix

        out = 0
        for mu, la, ls in self._loc_snapshot:
            out = out + local_covariance_matrix(self.data.wave, np.exp(la), mu, np.exp(ls))
        return out

    @_loc_cov.setter
    def _loc_cov(self, value):
        if value is not None:
            raise AttributeError("_loc_cov can only be reset to None")
        self._loc_snapshot = None

    # ------------------------------------------------------------------ parameter views
    @property
    def grid_params(self):
        """numpy.ndarray : emulator parameters in ``emulator.param_names`` order."""
        return np.array([self.params[key] for key in self.emulator.param_names])

    @grid_params.setter
    def grid_params(self, values):
        for key, value in zip(self.emulator.param_names, values):
            if key not in self.frozen:
                self.params[key] = value

    @property
    def cheb(self):
        """numpy.ndarray : c1, c2, ... (c0 is fixed to 1)."""
        return np.array(self.params["cheb"].values())

    @cheb.setter
    def cheb(self, values):
        if "cheb" in self.frozen:
            return
        for key, value in zip(self.params["cheb"], values):
            if key not in self.frozen:
                self.params["cheb"][key] = value

    @property
    def labels(self):
        """tuple of str : thawed parameter names, defining the meaning of a parameter vector."""
        return tuple(self.get_param_dict(flat=True).keys())

    def __getitem__(self, key):
        if key == "cheb":
            return list(self.params[key].values())
        return self.params[key]

    def __setitem__(self, key, value):
        if ":" in key:
            group, rest = key.split(":", 1)
            leaf = rest.split(":")[-1]
            if group == "global_cov" and leaf in self._GLOBAL_PARAMS:
                self.params[key] = value
            elif group == "local_cov" and leaf in self._LOCAL_PARAMS:
                self.params[key] = value
            elif group == "cheb":
                if "cheb" in self.params:
                    idx = int(rest)
                    if idx == 0:
                        raise KeyError("cannot change constant Chebyshev term")
                    for i in range(len(self.params[group]) + 1, idx + 1):
                        self.params[f"{group}:{i}"] = 0  # widen with zeros (spectrum_model.py:238-247)
                self.params[key] = value
            else:
                raise KeyError(f"{key} not recognized")
        elif key == "cheb":
            self.params[key] = {str(i): c for i, c in enumerate(value, start=1)}
        elif key in [*self._PARAMS, *self.emulator.param_names]:
            self.params[key] = value
        else:
            raise KeyError(f"{key} not recognized")

    def __delitem__(self, key):
        if key not in self.params:
            raise KeyError(f"{key} not in params")
        if key == "global_cov":
            self._glob_snapshot = None
            self.frozen = [k for k in self.frozen if not k.startswith("global_cov")]
        elif key == "local_cov":
            self._loc_snapshot = None
            self.frozen = [k for k in self.frozen if not k.startswith("local_cov")]
        del self.params[key]
        if key in self.frozen:
            self.frozen.remove(key)

    def get_param_dict(self, flat=False):
        """Thawed parameters, nested or flat (``'local_cov:0:mu'``)."""
        out = FlatterDict()
        for key, val in self.params.items():
            if key not in self.frozen:
                out[key] = val
        return out if flat else out.as_dict()

    def set_param_dict(self, params):
        """Update (never add) parameters; frozen keys are left untouched."""
        for key, val in FlatterDict(params).items():
            if key not in self.frozen:
                self.params[key] = val

    def get_param_vector(self):
        return np.array(list(self.get_param_dict(flat=True).values()))

    def set_param_vector(self, params):
        labels = self.labels
        if len(params) != len(labels):
            raise ValueError("Param Vector does not match length of thawed parameters")
        self.set_param_dict(dict(zip(labels, params)))

    # parameter groups: name -> attribute holding the hyper-parameter snapshot that freezing resets
    _GROUPS = {"global_cov": "_glob_snapshot", "local_cov": "_loc_snapshot", "cheb": None}

    def _group_members(self, group):
        """Flat keys stored below a group, in storage order ('local_cov:0:mu', 'cheb:2', ...)."""
        prefix = group + ":"
        return [key for key in self.params.keys() if key.startswith(prefix)]

    def freeze(self, names):
        """Remove parameters from the sampled vector; they keep their value (spectrum_model.py:495-549).
        A group name freezes all of its members and forgets the group's cached covariance; ``"all"``
        freezes everything that is thawed and keeps the caches."""
        names = [str(n) for n in np.atleast_1d(names)]
        if names[0] == "all":
            self.frozen += [key for key in self.labels if key not in self.frozen]
            self.frozen += [group for group in self._GROUPS if group in self.params]
            return
        for name in names:
            if name in self._GROUPS:
                self.frozen.append(name)
                if self._GROUPS[name]:
                    setattr(self, self._GROUPS[name], None)
                self.frozen += [key for key in self._group_members(name) if key not in self.frozen]
            elif name not in self.frozen and name in self.params:
                self.frozen.append(name)

    def thaw(self, names):
        """Opposite of :meth:`freeze` (spectrum_model.py:551-590); thawing a group that is not frozen
        raises ``ValueError`` like ``list.remove``."""
        names = [str(n) for n in np.atleast_1d(names)]
        if names[0] == "all":
            self.frozen = []
            return
        for name in names:
            if name in self._GROUPS:
                for key in [name, *self._group_members(name)]:
                    self.frozen.remove(key)
            elif name in self.frozen:
                self.frozen.remove(name)

    def _local_kernels(self):
        loc = self.params.as_dict().get("local_cov", [])
        return list(loc.values()) if isinstance(loc, dict) else list(loc)

    # ------------------------------------------------------------------ packing for the C-ABI
    def _model_desc(self, dev):
        """The C-ABI descriptor of the model's parameter rows.  ``dev`` None: built on the host, without a device."""
        n_local = len(self._local_kernels()) if "local_cov" in self.params else 0
        n_cheb = len(self.params["cheb"]) if "cheb" in self.params else 0
        make = dev.model_desc if dev is not None else (lambda *a, **k: D.DeviceOrder.model_desc(None, *a, **k))
        return make(
            "vsini" in self.params, "vz" in self.params, "log_scale" in self.params,
            "global_cov" in self.params, n_local, n_cheb, use_sigma_w=self.emulator_cov == "paper",
            has_av="Av" in self.params,
        )

    def _slot_of(self, dev, md):
        """flat parameter key -> column of the C-ABI parameter row (None: not used on the device).  ``dev`` None: the grid
        dimensions are the emulator's."""
        P = dev.P if dev is not None else len(self.emulator.param_names)
        slots = {"vsini": 0, "vz": 1, "log_scale": 2, "global_cov:log_amp": 4, "global_cov:log_ls": 5}
        for i, key in enumerate(self.emulator.param_names):
            slots[key] = 6 + i
        if "cheb" in self.params:
            for pos, key in enumerate(self.params["cheb"].keys()):  # positional, as [1, *self.cheb]
                slots[f"cheb:{key}"] = 6 + P + pos
        off_local = 6 + P + md.n_cheb
        for i in range(md.n_local):
            for j, leaf in enumerate(self._LOCAL_PARAMS):
                slots[f"local_cov:{i}:{leaf}"] = off_local + 3 * i + j
        if md.has_av:
            slots["Av"] = off_local + 3 * md.n_local  # Rv is accepted but never passed on (as the reference)
        return slots

    def _pack(self, P=None, update_caches=True):
        """Rows for the C-ABI.  ``P`` is None (current state, one row) or (B, len(labels))."""
        dev = self._device()
        md = self._model_desc(dev)
        slots = self._slot_of(dev, md)
        stride = dev.param_stride(md)
        base = np.zeros(stride)
        base[3] = 1.0
        for key, val in self.params.items():
            s = slots.get(key)
            if s is not None:
                base[s] = val
        if P is None:
            rows = base[None, :].copy()
        else:
            P = np.atleast_2d(np.asarray(P, dtype=np.float64))
            labels = self.labels
            if P.shape[1] != len(labels):
                raise ValueError("Param Vector does not match length of thawed parameters")
            rows = np.tile(base, (P.shape[0], 1))
            for col, key in enumerate(labels):
                s = slots.get(key)
                if s is not None:
                    rows[:, s] = P[:, col]
        if self.norm:  # spectrum_model.py:316-319
            g = rows[:, 6 : 6 + dev.P]
            rows[:, 3] = np.atleast_1d(self.emulator.norm_factor(g)).astype(np.float64)
        # frozen covariance groups keep the hyper-parameters seen when their cache was filled
        if md.has_global:
            if "global_cov" in self.frozen and self._glob_snapshot is not None:
                rows[:, 4:6] = self._glob_snapshot
            elif update_caches:
                self._glob_snapshot = tuple(rows[-1, 4:6])
        if md.n_local:
            lo = 6 + dev.P + md.n_cheb
            if "local_cov" in self.frozen and self._loc_snapshot is not None:
                rows[:, lo : lo + 3 * md.n_local] = np.asarray(self._loc_snapshot).reshape(-1)
            elif update_caches:
                self._loc_snapshot = [tuple(r) for r in rows[-1, lo : lo + 3 * md.n_local].reshape(-1, 3)]
        return dev, md, rows

    @staticmethod
    def _raise_for_info(code):
        code = int(code)
        if code > 0:
            raise np.linalg.LinAlgError(
                f"{code}-th leading minor of the array is not positive definite"
            )
        if code == -3:
            raise np.linalg.LinAlgError(D.INFO_MESSAGES[-3])
        if code == D.INFO_INTERNAL:  # (survived the retry of DeviceOrder.loglike: not a property of the parameters)
            raise RuntimeError(D.INFO_MESSAGES[D.INFO_INTERNAL])
        if code < 0:
            raise ValueError(D.INFO_MESSAGES.get(code, f"device status {code}"))

    # ------------------------------------------------------------------ evaluation
    def __call__(self):
        """(flux, cov) of the current state (spectrum_model.py:277-365); ``cov`` is a fresh N x N array."""
        dev, md, rows = self._pack()
        out = dev.forward(md, rows)
        self._raise_for_info(out["info"][0])
        self._log_scale = float(out["log_scale"][0])
        return out["flux"][0], out["cov"][0]

    def _prior(self, priors):
        lp = 0
        if priors is not None:
            for key, prior in priors.items():
                if key in self.params:
                    lp += prior.logpdf(self[key])
        return lp

    def log_likelihood(self, priors=None):
        """-(logdet + R^T C^-1 R)/2 + log-prior (spectrum_model.py:367-407)."""
        prior_lp = self._prior(priors)
        if not np.isfinite(prior_lp):
            return -np.inf
        dev, md, rows = self._pack()
        out = dev.loglike(md, rows, want_resid=True, solver=self.solver)
        self.last_info = out["info"]
        self._raise_for_info(out["info"][0])
        self._log_scale = float(out["log_scale"][0])
        self.residuals.append(out["resid"][0])
        self._lnprob = float(out["lnl"][0])
        return self._lnprob + prior_lp

    def _batch_prior(self, P, priors):
        """Log-prior of every row of ``P`` (labels order); parameters not in ``labels`` use the current value."""
        labels = self.labels
        prior_lp = np.zeros(P.shape[0])
        if priors:
            current = {k: self[k] for k in priors if k in self.params}
            for key, prior in priors.items():
                if key not in self.params:
                    continue
                if key in labels:
                    prior_lp += np.asarray(prior.logpdf(P[:, labels.index(key)]), dtype=np.float64)
                else:
                    prior_lp += prior.logpdf(current[key])
        return prior_lp

    def log_likelihood_batch(self, P, priors=None, return_info=False):
        """Log-posterior of B parameter vectors (rows of ``P`` in :attr:`labels` order) in one batched
        device pass.  Walkers that fail (outside the emulator grid, vsini <= 0, non-positive-definite
        covariance, non-finite prior) get ``-inf`` instead of raising; ``info`` carries the codes of
        include/starfish_amd.h.  The model's own parameter state is not modified."""
        P = np.atleast_2d(np.asarray(P, dtype=np.float64))
        prior_lp = self._batch_prior(P, priors)
        finite = np.isfinite(prior_lp)
        lnl = np.full(P.shape[0], -np.inf)
        info = np.zeros(P.shape[0], dtype=np.int32)
        if finite.any():
            # (update_caches=False: a batch must not overwrite the hyper-parameter snapshots that a later
            # freeze("all") + log_likelihood() of the model's OWN state relies on)
            dev, md, rows = self._pack(P[finite], update_caches=False)
            out = dev.loglike(md, rows, solver=self.solver)
            lnl[finite] = out["lnl"] + prior_lp[finite]
            info[finite] = out["info"]
        self.last_info = info
        return (lnl, info) if return_info else lnl

    # ------------------------------------------------------------------ the Cholesky factor of the covariance, applied
    # Diagnostics, not likelihood evaluations: none of them touches residuals, _lnprob, _log_scale or the covariance caches.
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
        dev, md, rows = self._pack(P, update_caches=False)
        return getattr(dev, call)(md, rows, *args, rhs=rhs, **kwargs), md, rhs, single

    def _own(self, out):
        """The first walker of a device result, or what :meth:`log_likelihood` raises for its status."""
        self._raise_for_info(out["info"][0])
        return {key: v[0] for key, v in out.items()}

    def _apply_factor(self, op, rhs, want_flux=False):
        """``op`` of :meth:`apply_factor_batch` for the current parameters; raises as :meth:`log_likelihood` does."""
        out, _, _, single = self._diagnose("apply", None, rhs, op, want_flux=want_flux)
        out = self._own(out)
        return (out["out"][0] if single else out["out"]), (out["flux"] if want_flux else None)

    def cho_solve(self, rhs=None):
        """``C^-1 rhs`` for the covariance of the current parameters, jitter included (the reference's
        ``cho_solve(factor, R)``, spectrum_model.py:404), solved on the device with the factor the likelihood uses.
        ``rhs``: (n,) or (k, n); None = the current residual ``flux - data.flux``."""
        return self._apply_factor("Cinv", rhs)[0]

    def whiten(self, rhs=None):
        """``L^-1 rhs`` (C = L L^T): iid N(0, 1) if ``rhs`` is noise drawn from C.  None = the current residual."""
        return self._apply_factor("Linv", rhs)[0]

    def draw(self, size=None, rng=None, z=None):
        """Noise realisations ``flux + L z`` of the current model.  Pass standard-normal ``z`` of shape (n,) or (k, n), or
        ``size`` (None: one draw of shape (n,); k: (k, n)) and ``rng`` (a ``numpy.random.Generator`` or a seed)."""
        n = len(self.data.wave)
        if z is None:
            gen = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
            z = gen.standard_normal(n if size is None else (int(size), n))
        elif size is not None:
            raise ValueError("pass either z or size, not both")
        lz, flux = self._apply_factor("L", z, want_flux=True)
        return flux + lz

    def apply_factor_batch(self, P, op, rhs=None, return_info=False):
        """The factor of B walkers' covariance matrices (rows of ``P`` in :attr:`labels` order) applied in one batched
        device pass: ``op`` "L" (L rhs), "Linv" (L^-1 rhs), "LinvT" (L^-T rhs) or "Cinv" (C^-1 rhs).  ``rhs``: None (each
        walker's own residual), (n,) / (k, n) shared by all walkers, or (B, k, n).  Returns (B, k, n) -- (B, n) for None
        or (n,) --; walkers that fail (outside the emulator grid, covariance not positive definite, ...) get NaN rows,
        ``info`` the codes of :meth:`log_likelihood_batch`.  The model's own state is not modified."""
        if op not in D.APPLY_OPS:
            raise ValueError(f"op must be one of {sorted(D.APPLY_OPS)}")
        out, _, _, single = self._diagnose("apply", np.atleast_2d(np.asarray(P, dtype=np.float64)), rhs, op)
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

    def residual_components(self, rhs=None):
        """The conditional mean of every covariance component given ``rhs`` (None: the current residual ``flux -
        data.flux``; (n,) or (k, n)): dict with "emulator", "noise", "global" (models with ``global_cov``), "local"
        (models with ``local_cov``: one row per kernel, in the order of ``self["local_cov"]``) and "alpha" = ``C^-1 rhs``
        (:meth:`cho_solve`).  The components add up to ``rhs``.  Raises as :meth:`log_likelihood` does."""
        out, md, _, single = self._diagnose("decompose", None, rhs)
        out = self._own(out)
        return self._component_dict(out["comp"], out["alpha"], bool(md.has_global), int(md.n_local), single)

    def residual_components_batch(self, P, rhs=None, return_info=False):
        """:meth:`residual_components` for B walkers (rows of ``P`` in :attr:`labels` order) in one batched device pass:
        the same keys with a leading B axis.  ``rhs`` as for :meth:`apply_factor_batch`; walkers that fail get NaN rows,
        ``info`` their codes.  The model's own state is not modified."""
        out, md, _, single = self._diagnose("decompose", np.atleast_2d(np.asarray(P, dtype=np.float64)), rhs)
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

    def pointwise(self, rhs=None):
        """Every pixel of ``rhs`` (None: the current residual ``flux - data.flux``; (n,) or (k, n)) judged against the
        prediction from all the OTHER pixels under the covariance of the current parameters: dict with "alpha" = ``C^-1
        rhs`` (:meth:`cho_solve`), "marginal_std" = ``sqrt(diag(C))`` (jitter included; the band the reference's plot
        shades), "loo_mean" = ``rhs - alpha / d`` and "loo_std" = ``1 / sqrt(d)`` with ``d = diag(C^-1)``, the
        standardised residual "z" = ``alpha / sqrt(d)`` and the per-pixel "log_density" = ``-log(2 pi / d) / 2 - z^2 / 2``,
        whose sum is the leave-one-out pseudo-likelihood.  "marginal_std" and "loo_std" are (n,) whatever ``rhs`` is.
        Raises as :meth:`log_likelihood` does."""
        out, _, rhs, single = self._diagnose("pointwise", None, rhs, want_flux=rhs is None)
        out = self._own(out)
        if rhs is None:
            rhs = (out["flux"] - self.data.flux)[None, :]
        return self._pointwise_dict(rhs, out["alpha"], out["cinv_diag"], out["cov_diag"], single)

    def pointwise_batch(self, P, rhs=None, return_info=False):
        """:meth:`pointwise` for B walkers (rows of ``P`` in :attr:`labels` order) in one batched device pass: the same
        keys with a leading B axis.  ``rhs`` as for :meth:`apply_factor_batch`; walkers that fail get NaN rows, ``info``
        their codes.  The model's own state is not modified."""
        out, _, rhs, single = self._diagnose("pointwise", np.atleast_2d(np.asarray(P, dtype=np.float64)), rhs,
                                             want_flux=rhs is None)
        if rhs is None:
            rhs = (out["flux"] - self.data.flux)[:, None, :]
        res = self._pointwise_dict(rhs, out["alpha"], out["cinv_diag"], out["cov_diag"], single)
        return (res, out["info"]) if return_info else res

    # ------------------------------------------------------------------ gradient in the covariance hyper-parameters
    @property
    def gradient_labels(self):
        """tuple of str : the thawed labels under ``global_cov:`` / ``local_cov:``, in :attr:`labels` order: the parameters
        :meth:`log_likelihood_gradient` differentiates in."""
        return tuple(key for key in self.labels if key.startswith(("global_cov:", "local_cov:")))

    def _gradient_slots(self, md):
        """For every label of :attr:`gradient_labels`, its slot in the device's gradient row (log_amp, log_ls of the global
        kernel if the model has one, then mu, log_amp, log_sigma per local kernel)."""
        first_local = 2 if md.has_global else 0
        slots = []
        for key in self.gradient_labels:
            group, rest = key.split(":", 1)
            if group == "global_cov":
                slots.append(self._GLOBAL_PARAMS.index(rest))
            else:
                i, leaf = rest.split(":")
                slots.append(first_local + 3 * int(i) + self._LOCAL_PARAMS.index(leaf))
        return slots

    def log_likelihood_gradient(self):
        """``(lnL, {label: d lnL / d label})`` of the current state for the labels of :attr:`gradient_labels`: the analytic
        gradient of :meth:`log_likelihood` (no priors) in the covariance hyper-parameters, from one factorisation
        (Rasmussen & Williams, GPML, eq. 5.9).  In ``mu`` of a local kernel it is the almost-everywhere derivative: the
        likelihood has a kink wherever two pixels of the patch are equidistant from ``mu``.  Raises as
        :meth:`log_likelihood` does; the model's state is not modified."""
        labels = self.gradient_labels
        if not labels:
            raise ValueError("no thawed global_cov / local_cov parameter to differentiate in")
        dev, md, rows = self._pack(update_caches=False)
        out = self._own(dev.loglike_grad(md, rows))
        return float(out["lnl"]), dict(zip(labels, (float(v) for v in out["grad"][self._gradient_slots(md)])))

    def log_likelihood_gradient_batch(self, P, return_info=False):
        """:meth:`log_likelihood_gradient` for B walkers (rows of ``P`` in :attr:`labels` order) in one batched device pass:
        ``(lnL (B,), grad (B, len(gradient_labels)))``.  Walkers that fail get ``-inf`` and a NaN row, ``info`` their codes.
        The model's own state is not modified."""
        if not self.gradient_labels:
            raise ValueError("no thawed global_cov / local_cov parameter to differentiate in")
        P = np.atleast_2d(np.asarray(P, dtype=np.float64))
        dev, md, rows = self._pack(P, update_caches=False)
        out = dev.loglike_grad(md, rows)
        lnl = np.where(out["info"] == 0, out["lnl"], -np.inf)
        grad = out["grad"][:, self._gradient_slots(md)]
        return (lnl, grad, out["info"]) if return_info else (lnl, grad)

    def train_covariance(self, priors=None, **kwargs):
        """MAP estimate of the covariance hyper-parameters alone: ``scipy.optimize.minimize(method="L-BFGS-B", jac=True)``
        over :attr:`gradient_labels` with the analytic gradient of :meth:`log_likelihood_gradient_batch`; every other
        parameter keeps its value.  ``priors`` are checked as :meth:`train` checks them; a prior on an optimised label adds
        its ``logpdf`` and the slope of it by a central difference with step ``eps^(1/3) max(1, |x|)`` (scipy's frozen
        distributions expose no derivative), priors on other parameters a constant.  ``kwargs`` go to ``minimize``.  On
        success the model is left at ``soln.x``."""
        from scipy.optimize import minimize

        priors = self._checked_priors(priors)
        glabels = self.gradient_labels
        if not glabels:
            raise ValueError("no thawed global_cov / local_cov parameter to optimise")
        labels = self.labels
        cols = [labels.index(key) for key in glabels]
        x_all = self.get_param_vector().astype(np.float64)
        const_lp = sum(prior.logpdf(self[key]) for key, prior in priors.items() if key in self.params and key not in glabels)
        h0 = np.finfo(np.float64).eps ** (1.0 / 3.0)

        def objective(x):
            row = x_all.copy()
            row[cols] = x
            lnl, grad, info = self.log_likelihood_gradient_batch(row[None, :], return_info=True)
            self._raise_for_info(info[0])
            value, slope = float(lnl[0]) + const_lp, grad[0].copy()
            for i, key in enumerate(glabels):
                if key in priors:
                    h = h0 * max(1.0, abs(x[i]))
                    value += priors[key].logpdf(x[i])
                    slope[i] += (priors[key].logpdf(x[i] + h) - priors[key].logpdf(x[i] - h)) / (2 * h)
            return -value, -slope

        opts = {"method": "L-BFGS-B", "jac": True}
        opts.update(kwargs)
        soln = minimize(objective, x_all[cols], **opts)
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

    def log_likelihood_mean_gradient(self):
        """``(lnL, {label: d lnL / d label})`` of the current state for the labels of :attr:`mean_gradient_labels`: the analytic
        gradient of :meth:`log_likelihood` (no priors) in vsini, vz, log_scale, Av, the Chebyshev coefficients and the grid
        parameters, from the likelihood's factorisation and one solve with 1 + m right-hand sides.  Raises as
        :meth:`log_likelihood` does; the model's state is not modified."""
        dev, md, rows = self._pack(update_caches=False)
        out = self._own(dev.loglike_mean_grad(md, rows, self._mean_gradient_columns(dev, md)))
        return float(out["lnl"]), dict(zip(self.mean_gradient_labels, (float(v) for v in out["grad"])))

    def log_likelihood_mean_gradient_batch(self, P, return_info=False):
        """:meth:`log_likelihood_mean_gradient` for B walkers (rows of ``P`` in :attr:`labels` order) in one batched device
        pass: ``(lnL (B,), grad (B, len(mean_gradient_labels)))``.  Walkers that fail get ``-inf`` and a NaN row, ``info`` their
        codes.  The model's own state is not modified."""
        P = np.atleast_2d(np.asarray(P, dtype=np.float64))
        dev, md, rows = self._pack(P, update_caches=False)
        out = dev.loglike_mean_grad(md, rows, self._mean_gradient_columns(dev, md))
        lnl = np.where(out["info"] == 0, out["lnl"], -np.inf)
        return (lnl, out["grad"], out["info"]) if return_info else (lnl, out["grad"])

    def log_likelihood_full_gradient_batch(self, P, return_info=False, one_pass=False):
        """``(lnL (B,), grad (B, len(labels)))``: the gradient in every thawed label, columns in :attr:`labels` order -- the mean
        call's columns and, where covariance labels are thawed, :meth:`log_likelihood_gradient_batch`'s (two device calls).  A
        thawed ``Rv`` gets a zero column: it is never passed on.

        ``one_pass=True``: both parts from ONE factorisation per walker (sf_loglike_multi_grad_batch_md with one segment)
        instead of one per call; the values agree with the default's to rounding, not bit for bit."""
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
            out = D.loglike_multi_grad([dev], [md], [rows], [(columns, bool(cov))])[0]
            grad[:, [labels.index(key) for key in mean]] = out["grad"][:, :len(columns)]
            if cov:
                grad[:, [labels.index(key) for key in cov]] = out["grad"][:, [len(columns) + s for s in self._gradient_slots(md)]]
            lnl, info = np.where(out["info"] == 0, out["lnl"], -np.inf), out["info"]
            return (lnl, grad, info) if return_info else (lnl, grad)
        if self.mean_gradient_labels:
            lnl, g, info = self.log_likelihood_mean_gradient_batch(P, return_info=True)
            grad[:, [labels.index(key) for key in self.mean_gradient_labels]] = g
        if self.gradient_labels:
            lnl, g, info = self.log_likelihood_gradient_batch(P, return_info=True)
            grad[:, [labels.index(key) for key in self.gradient_labels]] = g
        if lnl is None:
            raise ValueError("no thawed parameter to differentiate in")
        return (lnl, grad, info) if return_info else (lnl, grad)

    def _checked_priors(self, priors):
        """``priors`` ({} for None) after the checks of :meth:`train` (spectrum_model.py:655-668)."""
        priors = {} if priors is None else priors
        for key, val in priors.items():
            if key not in self.params and not key.startswith("cheb"):
                raise ValueError(f"Invalid priors: {key!r} is not a parameter of this model")
            if not callable(getattr(val, "logpdf", None)):
                raise ValueError(f"Invalid priors. {key} does not have a `logpdf` method")
            log_prob = val.logpdf(self[key])
            if not np.isfinite(log_prob):
                raise RuntimeError(f"{key}'s logpdf evaluated to {log_prob}")
        return priors

    def train(self, priors=None, batch_simplex=True, gradient=False, **kwargs):
        """MAP estimate by Nelder-Mead over :meth:`log_likelihood` (spectrum_model.py:635-696).  ``kwargs`` go to
        ``scipy.optimize.minimize`` as in the reference.

        With ``gradient=True`` the search is ``minimize(method="L-BFGS-B", jac=True)`` over all of :attr:`labels` on the analytic
        gradient of :meth:`log_likelihood_full_gradient_batch`; priors and their slopes are handled as in
        :meth:`train_covariance`, a point the device flags raises as :meth:`log_likelihood` does, every evaluation leaves the
        model at its point, a run that succeeds or stops at its iteration limit at ``soln.x``; ``batch_simplex`` plays no part then.  Without it the path below is
        unchanged.

        The reference's loop is ~10^3 SERIAL scalar evaluations.  Here (``batch_simplex=True``, a plain Nelder-Mead run:
        no other ``method``, no bounds) the candidate points of every simplex iteration -- reflection, expansion, both
        contractions: all functions of the current simplex -- are evaluated as ONE device batch of four, the initial
        simplex and every shrink step as one batch each (:mod:`starfish_amd._neldermead`); the accept / contract / shrink
        decisions, their order, ``nit`` / ``nfev`` / ``status`` and the exceptions of invalid points are scipy's.  The
        state the model is left in is the reference's too: the parameters, caches, ``residuals`` entry and
        ``_lnprob`` of the LAST point the objective was asked for, then ``soln.x`` if the run succeeded."""
        from scipy.optimize import minimize

        from .._neldermead import minimize_neldermead_batched, split_minimize_kwargs

        priors = self._checked_priors(priors)
        if gradient:
            return self._train_gradient(minimize, priors, kwargs)

        def nll(P):
            self.set_param_vector(P)
            return -self.log_likelihood(priors)

        nm_opts, why_not = split_minimize_kwargs(kwargs) if batch_simplex else (None, "batch_simplex=False")
        if nm_opts is None:
            self.log.debug(f"train: serial scipy path ({why_not})")
            opts = {"method": "Nelder-Mead"}
            opts.update(kwargs)
            soln = minimize(nll, self.get_param_vector(), **opts)
        else:
            def nll_batch(X):
                lnl, info = self.log_likelihood_batch(X, priors, return_info=True)

                def raiser(i):  # the scalar objective raises for these (spectrum_model.py:400, emulator.py:377-378, ...)
                    self._raise_for_info(info[i])

                return -lnl, raiser

            soln = minimize_neldermead_batched(nll_batch, self.get_param_vector(), **nm_opts)
            # leave the model where the reference's last objective call left it (parameters, frozen-cache snapshots, the
            # residual deque, _lnprob): ONE scalar evaluation at that point
            nll(soln.last_x)
        if soln.success:
            self.set_param_vector(soln.x)
        return soln

    def _train_gradient(self, minimize, priors, kwargs):
        """The ``gradient=True`` search of :meth:`train`."""
        labels = self.labels
        const_lp = sum(prior.logpdf(self[key]) for key, prior in priors.items() if key in self.params and key not in labels)
        h0 = np.finfo(np.float64).eps ** (1.0 / 3.0)

        def objective(x):
            if np.any(~np.isfinite(x)):
                raise ValueError("SpectrumModel.train: the optimiser asked for a point that is not finite")
            self.set_param_vector(x)
            lnl, grad, info = self.log_likelihood_full_gradient_batch(x[None, :], return_info=True)
            self._raise_for_info(info[0])
            value, slope = float(lnl[0]) + const_lp, grad[0].copy()
            for i, key in enumerate(labels):
                if key in priors:
                    h = h0 * max(1.0, abs(x[i]))
                    value += priors[key].logpdf(x[i])
                    slope[i] += (priors[key].logpdf(x[i] + h) - priors[key].logpdf(x[i] - h)) / (2 * h)
            return -value, -slope

        opts = {"method": "L-BFGS-B"}
        opts.update(kwargs)
        opts["jac"] = True
        soln = minimize(objective, self.get_param_vector().astype(np.float64), **opts)
        if soln.success or soln.status == 1:  # (1: the iteration / evaluation limit; soln.x is the best point so far)
            self.set_param_vector(soln.x)
        return soln

    # ------------------------------------------------------------------ persistence
    def save(self, filename, metadata=None):
        """Write parameters / frozen list / metadata as TOML (spectrum_model.py:592-619)."""
        from .._toml import dumps

        meta = {"name": self.name, "data": self.data_name}
        if self.emulator.name is not None:
            meta["emulator"] = self.emulator.name
        if metadata is not None:
            meta.update(metadata)
        doc = {"parameters": self.params.as_dict(), "frozen": list(self.frozen), "metadata": meta}
        with open(filename, "w") as fh:
            fh.write(dumps(doc))
        self.log.info(f"Saved current state at {filename}")

    def load(self, filename):
        """Read a state written by :meth:`save` (spectrum_model.py:621-633)."""
        from .._toml import load

        data = load(filename)
        self.params = FlatterDict(data["parameters"])
        self.frozen = list(data["frozen"])
        self._glob_snapshot = None
        self._loc_snapshot = None

    def plot(self, *args, **kwargs):
        raise NotImplementedError("plotting is out of scope for the MI355X hot path")

    def __repr__(self):
        out = f"{self.name}\n" + "-" * len(self.name) + "\n"
        out += f"Data: {self.data_name}\n"
        out += f"Emulator: {self.emulator.name}\n"
        out += f"Log Likelihood: {self._lnprob}\n"
        out += "\nParameters\n"
        for key, value in self.get_param_dict().items():
            if key == "global_cov":
                out += "  global_cov:\n"
                for gkey, gval in value.items():
                    out += f"    {gkey}: {gval}\n"
            elif key == "local_cov":
                out += "  local_cov:\n"
                kernels = value.values() if isinstance(value, dict) else value
                for i, kern in enumerate(kernels):
                    out += f"    {i}: " + ", ".join(f"{k}: {v}" for k, v in kern.items()) + "\n"
            elif key == "cheb":
                out += f"  cheb: {list(value.values())}\n"
            else:
                out += f"  {key}: {value}\n"
        if "log_scale" not in self.params and self._log_scale is not None:
            out += f"  log_scale: {self._log_scale} (fit)\n"
        if self.frozen:
            out += "\nFrozen Parameters\n"
            for key in self.frozen:
                if key in ("global_cov", "local_cov", "cheb"):
                    continue
                out += f"  {key}: {self[key]}\n"
        return out[:-1]
