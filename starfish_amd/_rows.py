"""
THE Python statement of the C-ABI parameter row (include/starfish_amd.h): ``[0] vsini, [1] vz, [2] log_scale, [3] norm,
[4:6] global log_amp, log_ls``, then the grid parameters, the Chebyshev coefficients, ``mu, log_amp, log_sigma`` per local
kernel and Av.  Pure host logic; the row's length is ``sf_param_stride``'s to say, not this module's.
"""
from ._lib import ModelDesc

VSINI, VZ, LOG_SCALE, NORM, GLOBAL_LOG_AMP, GLOBAL_LOG_LS = range(6)
GLOBAL = slice(GLOBAL_LOG_AMP, GLOBAL_LOG_LS + 1)
GLOBAL_LEAVES = ("log_amp", "log_ls")
LOCAL_LEAVES = ("mu", "log_amp", "log_sigma")


def model_desc(has_vsini, has_vz, has_log_scale, has_global, n_local, n_cheb, use_sigma_w=False, has_av=False):
    """The C-ABI descriptor of a model's parameter rows."""
    md = ModelDesc()
    md.has_vsini, md.has_vz = int(has_vsini), int(has_vz)
    md.has_log_scale, md.has_global = int(has_log_scale), int(has_global)
    md.n_local, md.n_cheb, md.use_sigma_w = int(n_local), int(n_cheb), int(use_sigma_w)
    md.has_av = int(has_av)
    return md


class RowLayout:
    """The columns behind the fixed ones for ``P`` grid parameters and the descriptor ``md``: the slices ``grid``, ``cheb``
    and ``local`` (:meth:`local_of` kernel i's three) and the column ``av`` (None without Av)."""

    def __init__(self, P, md):
        self.grid = slice(GLOBAL.stop, GLOBAL.stop + int(P))
        self.cheb = slice(self.grid.stop, self.grid.stop + int(md.n_cheb))
        self.local = slice(self.cheb.stop, self.cheb.stop + len(LOCAL_LEAVES) * int(md.n_local))
        self.av = self.local.stop if md.has_av else None

    def local_of(self, i):
        lo = self.local.start + len(LOCAL_LEAVES) * int(i)
        return slice(lo, lo + len(LOCAL_LEAVES))


def cov_grad_slots(md):
    """Length of the device's covariance-gradient row: log_amp, log_ls of the global kernel if the model has one, then mu,
    log_amp, log_sigma per local kernel."""
    return (len(GLOBAL_LEAVES) if md.has_global else 0) + len(LOCAL_LEAVES) * int(md.n_local)


def cov_grad_slot(md, label):
    """The slot of ``global_cov:<leaf>`` or ``local_cov:<i>:<leaf>`` in that row."""
    group, rest = label.split(":", 1)
    if group == "global_cov":
        return GLOBAL_LEAVES.index(rest)
    i, leaf = rest.split(":")
    return (len(GLOBAL_LEAVES) if md.has_global else 0) + len(LOCAL_LEAVES) * int(i) + LOCAL_LEAVES.index(leaf)
