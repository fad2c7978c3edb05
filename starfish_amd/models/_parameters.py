"""The parameter book of :class:`SpectrumModel`: the FlatterDict store, labels, freeze / thaw, TOML persistence, repr.  No
device in here."""
import numpy as np

from .. import _rows as R
from .._flatdict import FlatterDict


class ParameterBook:
    _PARAMS = ["vz", "vsini", "Av", "Rv", "log_scale", "global_cov", "local_cov", "cheb"]
    _GLOBAL_PARAMS = list(R.GLOBAL_LEAVES)
    _LOCAL_PARAMS = list(R.LOCAL_LEAVES)

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
