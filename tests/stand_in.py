"""A stand-in for DeviceOrder under the ``*_host.py`` tests: SpectrumModel's host logic on the CPU.  The descriptor and the row
stride are written out here on purpose: they are the tests' own statement of the C-ABI row, not the package's."""
from starfish_amd import _lib, synth


class StandIn:
    """What every SpectrumModel method asks of a DeviceOrder; a test adds the fake device calls it needs in a subclass."""

    def __init__(self, n, info=0):
        self.n, self.P, self.info, self.calls = n, 3, info, []

    def model_desc(self, has_vsini, has_vz, has_log_scale, has_global, n_local, n_cheb, use_sigma_w=False, has_av=False):
        md = _lib.ModelDesc()
        md.has_vsini, md.has_vz, md.has_log_scale, md.has_global = int(has_vsini), int(has_vz), int(has_log_scale), int(has_global)
        md.n_local, md.n_cheb, md.use_sigma_w, md.has_av = int(n_local), int(n_cheb), int(use_sigma_w), int(has_av)
        return md

    def param_stride(self, md):
        return 6 + self.P + md.n_cheb + 3 * md.n_local + md.has_av


def model_on_a_stand_in(cls, N=64, params=None, **kw):
    """``(model, standin)``: a synthetic order's model on ``cls(N)``.  ``params``: None (the centre of the walker ball), a dict
    laid over it, or ``order -> dict``; ``kw`` go to ``synth.build_model``."""
    o = synth.make_order(N=N, m=3, seed=9)
    if params is not None:
        params = params(o) if callable(params) else dict(synth.centre_params(o), **params)
    model = synth.build_model(o, params=params, **kw)
    standin = cls(N)
    model._device = lambda: standin
    return model, standin


def state_of(model):
    return (len(model.residuals), model._lnprob, model._log_scale, model._glob_snapshot, model._loc_snapshot,
            tuple(model.get_param_vector()), tuple(model.frozen))
