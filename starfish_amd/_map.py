"""
THE maximum-a-posteriori search of the trainers that have an analytic likelihood gradient: L-BFGS-B over ``(-value, -slope)``
with the log-priors of the optimised labels and their slopes added.  What each trainer does differently is an argument here
or code of the caller ("Python layer", has the table).
"""
import numpy as np

_H0 = np.finfo(np.float64).eps ** (1.0 / 3.0)


def prior_value_and_slope(prior, x):
    """``prior.logpdf(x)`` and its slope by a central difference with step ``eps^(1/3) max(1, |x|)`` (scipy's frozen
    distributions expose no derivative)."""
    h = _H0 * max(1.0, abs(x))
    return prior.logpdf(x), (prior.logpdf(x + h) - prior.logpdf(x - h)) / (2 * h)


def minimize_lbfgsb(evaluate, x0, sampled, const_lp, kwargs, finite_for=None, force_jac=True):
    """``scipy.optimize.minimize`` of ``-(lnL + log-prior)``.  ``evaluate(x) -> (lnl, grad)`` raises for a point the device
    flags; ``sampled``: ``(column of x, prior)`` of every prior on an optimised label, added in that order behind
    ``const_lp``, the priors on everything else.  A caller without priors, or one whose ``evaluate`` returns the posterior
    and its slope already, passes ``[]`` and None: nothing is added then, not even a zero.  ``kwargs`` are the caller's for ``minimize``: they may replace the method;
    ``jac=True`` is forced unless ``force_jac`` is False, which lets them replace that too.  ``finite_for``: the name under
    which a point that is not finite raises ``ValueError`` (None: no check).  Returns scipy's result; what becomes of
    ``soln.x`` is the caller's business."""
    from scipy.optimize import minimize

    def objective(x):
        if finite_for and np.any(~np.isfinite(x)):
            raise ValueError(f"{finite_for}: the optimiser asked for a point that is not finite")
        lnl, grad = evaluate(x)
        value, slope = float(lnl), np.array(grad, dtype=np.float64)
        if const_lp is not None:
            value += const_lp
        for col, prior in sampled:
            v, s = prior_value_and_slope(prior, x[col])
            value += v
            slope[col] += s
        return -value, -slope

    opts = {"method": "L-BFGS-B", "jac": True}
    opts.update(kwargs)
    if force_jac:
        opts["jac"] = True
    return minimize(objective, x0, **opts)


def laplace_covariance(fisher, labels, terms):
    """The Laplace covariance of ``labels`` from their Fisher matrix: ``terms`` lists ``(position, prior, x)`` for every prior on
    one of the labels, and each adds ``-d^2 logpdf / d x^2`` at ``x`` to its diagonal entry by a central second difference with
    the step of :func:`prior_value_and_slope`, in the order given.  The inverse is formed in normalised form, ``D^-1 (D^-1 F
    D^-1)^-1 D^-1`` with ``D = sqrt(diag(F))``, by Cholesky; a matrix that is not positive definite (parameters the data do not
    separate) raises ``np.linalg.LinAlgError`` naming the labels."""
    F = np.array(fisher, dtype=np.float64)
    for i, prior, x in terms:
        h = _H0 * max(1.0, abs(x))
        lp = prior.logpdf
        F[i, i] -= (lp(x + h) - 2.0 * lp(x) + lp(x - h)) / (h * h)
    with np.errstate(invalid="ignore"):  # (a negative diagonal entry: NaN, refused below)
        d = np.sqrt(np.diag(F))
    if not (np.all(np.isfinite(F)) and np.all(d > 0)):
        raise np.linalg.LinAlgError(f"the Fisher matrix of {list(labels)} has a diagonal entry that is not positive or an "
                                    "entry that is not finite")
    try:
        L = np.linalg.cholesky(F / np.outer(d, d))
    except np.linalg.LinAlgError:
        raise np.linalg.LinAlgError(f"the Fisher matrix of {list(labels)} is not positive definite: the data (and priors) do "
                                    "not separate these parameters; freeze some of them or add priors") from None
    Li = np.linalg.solve(L, np.eye(len(labels)))
    return (Li.T @ Li) / np.outer(d, d)
