"""Inputs and error bounds of the multi-order gradient tests (sf_loglike_multi_grad_batch_md, EchelleModel's gradient).

Inputs.  Case A: per_order_models((0, 1, 3), sizes=[64, 130, 180], m=2, seed0=100) -- common npad 192 (the factorisation's
shifted frame), the 64-pixel order beside a 128-row identity block, the 130-pixel order with 2 rows in its last block.
Case B: per_order_models((3, 0, 1), sizes=[180, 64, 256], m=4, seed0=100) -- common npad 256.  Both as
EchelleModel.from_orders(models, per_order=PER) (32 labels) with the three walkers of per_order_cases.ball(em, 3, seed=1).

Bounds.  The two derived bounds of tests/test_gpu_gradient.py (covariance slots, its docstring items 1-4) and
tests/test_gpu_mean_gradient.py (mean slots, items 1-4) are restated here, since those files do not export them, against the
same np.longdouble references (tests/cov_derivatives.py, tests/mean_derivatives.py).  N is the order's own number of pixels,
n the npad of the call (the group's common one): the padding enters the rounding constants gamma_{n+1} and gamma_{2n} only.
Where those bounds use the device's own factor L and X = L^-1, the longdouble Cholesky factor of the reference matrix padded
with the identity is used here -- the multi-order call does not hand the factor out; its data block is the factor of the
reference matrix itself and the identity block adds nothing to |L||L|^T, |X|^T|X| or E on the data rows, so the N x N factor
is what is formed.  The two factors differ in second order of the rounding.  Both wrong-weight guards stay the hard
assertion: agreement with the float64 helper to 1e-6 of the sum of absolute values."""
import numpy as np

from oracle import sf_oracle as O
from per_order_cases import PER, ball, oracle_params, per_order_models
from starfish_amd.models import EchelleModel

import cov_derivatives as CD
import mean_derivatives as MD

U = 2.0 ** -53
LD = np.longdouble
CASES = {"A": ((0, 1, 3), [64, 130, 180], 2, 192), "B": ((3, 0, 1), [180, 64, 256], 4, 256)}


def gamma(k):
    return k * U / (1 - k * U)


def build(name):
    """(orders, models, em, P) of a case; no device is touched."""
    n_local, sizes, m, _ = CASES[name]
    orders, models = per_order_models(n_local, sizes=list(sizes), m=m, seed0=100)
    em = EchelleModel.from_orders(models, per_order=PER)
    return orders, models, em, ball(em, 3, seed=1)


def kink_distances(wave, p):
    """For every local kernel of the oracle parameter dict ``p``: the distance of its mu, in pixels, from the nearest pixel or
    midpoint of two pixels (where the likelihood has a kink in mu)."""
    w = np.asarray(wave)
    mids = 0.5 * (w[:, None] + w[None, :])  # (the diagonal: the pixels themselves)
    out = []
    for mu, _, _ in p.get("local_cov", []):
        k = int(np.clip(np.searchsorted(w, mu), 1, len(w) - 1))
        out.append(float(np.abs(mids - mu).min() / (w[k] - w[k - 1])))
    return out


def inverse_longdouble(L):
    X = np.zeros_like(L)
    for i in range(L.shape[0]):
        row = -(L[i, :i] @ X[:i])
        row[i] += 1
        X[i] = row / L[i, i]
    return X


def cholesky_longdouble(A):
    L = np.zeros_like(A)
    for j in range(A.shape[0]):
        L[j, j] = np.sqrt(A[j, j] - L[j, :j] @ L[j, :j])
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def check_cov_slots(tag, oo, p, flux, npad, got):
    """Every covariance slot of one unit (``got``, device order) within the bound of tests/test_gpu_gradient.py.  flux: the
    device's own model flux of the unit; npad: the call's.  Prints err / bound per slot; returns the largest ratio."""
    N, wave = len(oo.wave), oo.wave
    C64 = O.forward_model(oo, p)[1] + 1e-10 * np.eye(N)
    Lr = cholesky_longdouble(C64.astype(LD))
    Xr = inverse_longdouble(Lr)
    Cinv = Xr.T @ Xr
    r64 = flux - oo.flux
    alpha = Cinv @ r64.astype(LD)
    A = np.outer(alpha, alpha) - Cinv
    aL, aX = np.abs(Lr).astype(np.float64), np.abs(Xr).astype(np.float64)
    aCi, aal, aA = np.abs(Cinv).astype(np.float64), np.abs(alpha).astype(np.float64), np.abs(A).astype(np.float64)
    dC = 1e-13 * np.abs(C64) + gamma(npad + 1) * (aL @ aL.T)
    solve = (1e-13 + N * gamma(3 * N + 1)) * (np.abs(C64).sum(axis=1).max() * aal.max() + np.abs(r64).max())
    d_alpha = aCi @ (dC @ aal) + aCi.sum(axis=1) * solve
    E = aX.T @ (aX @ (aL @ aX))
    dG = aCi @ dC @ aCi + gamma(2 * npad) * (E + E.T) + gamma(npad + 1) * (aX.T @ aX)
    first = np.outer(d_alpha, aal) + np.outer(aal, d_alpha) + dG
    second = 3 * U * (np.outer(aal, aal) + aCi)
    A64 = np.outer(*(np.linalg.solve(C64, r64),) * 2) - np.linalg.inv(C64)  # the float64 reference of the wrong-weight guard
    D = CD.slot_derivatives(wave, p, dtype=LD)
    Dbar = CD.slot_derivatives(wave, p, absolute=True)
    D64 = CD.slot_derivatives(wave, p)
    assert len(D) == len(got), (tag, len(D), len(got))
    worst = 0.0
    for s, ((label, d), (_, dbar), (_, d64)) in enumerate(zip(D, Dbar, D64)):
        ref = 0.5 * np.sum(A * d)
        size = 0.5 * np.sum(aA * dbar)
        k = int(np.count_nonzero(dbar))
        bound = 0.5 * np.sum(first * dbar) + 0.5 * np.sum(second * dbar) + 1e-13 * size + gamma(k) * size
        err = abs(float(got[s] - ref))
        ref64 = 0.5 * np.sum(A64 * d64)
        print(f"{tag} {label}: {got[s]!r}, err / bound = {err / bound:.3g} (bound {bound:.3g}, {k} entries), "
              f"|got - float64 reference| / (1/2 sum |A| Dbar) = {abs(got[s] - ref64) / size:.3g}")
        assert abs(got[s] - ref64) <= 1e-6 * size, (tag, label, got[s], ref64, size)
        assert err <= bound, (tag, label, got[s], float(ref), err, bound)
        worst = max(worst, err / bound)
    return worst


def check_mean_slots(tag, oo, p, flux, labels, got):
    """Every mean slot of one unit (``got[j]`` belongs to ``labels[j]``) within the bound of tests/test_gpu_mean_gradient.py.
    Prints err / bound per slot; returns the largest ratio."""
    N, m = len(oo.wave), oo.m
    fac = 1e-13 + N * gamma(3 * N + 1)
    ref64 = MD.gradient(oo, p, labels)
    q = {}
    refld = MD.gradient(oo, p, labels, dtype=LD, flux=flux, pieces=q)
    own64 = MD.gradient(oo, p, labels, flux=flux)
    ab = lambda v: np.abs(v).astype(np.float64)  # noqa: E731
    aCi, aX, aSi, aal, aza = np.abs(np.linalg.inv(q["C"])), ab(q["X"]), ab(q["Sinv"]), ab(q["alpha"]), ab(q["za"])
    cnorm, rowsum = np.abs(q["C"]).sum(axis=1).max(), aCi.sum(axis=1)
    d_alpha = rowsum * fac * (cnorm * aal.max() + ab(q["r"]).max())
    d_V = np.stack([rowsum * fac * (cnorm * ab(q["V"][:, k]).max() + aX[k].max()) for k in range(m)], axis=1)
    omega = np.outer(aal, aza) + ab(q["W"])  # (N, m)
    worst = 0.0
    for j, label in enumerate(labels):
        kind, d0, d1 = q["tan"][label]
        d0, d1 = np.abs(d0), np.abs(d1)
        sq = float(refld[label][1])
        if kind == "rows":
            solve = (d_alpha @ (d0 + d1.T @ aza) + np.sum(d1.T * np.outer(aal, aSi @ (aX @ d_alpha)))
                     + np.sum(d1.T * (d_V @ aSi)))
            contract = 1e-10 * (d0.max() * aal.sum() + d1.max() * omega.sum())
            k = N * (1 + 2 * m)
        else:
            da = aX @ d_alpha
            solve = d0 @ da + aza @ (d1 @ (aSi @ da)) + 0.5 * np.sum(d1 * (aSi @ (aX @ d_V) @ aSi))
            contract = 0.0
            k = m + 2 * m * m
        other_order = 8 * abs(float(own64[label][0] - refld[label][0]))
        bound = solve + contract + (gamma(k) + 3 * U) * sq + other_order + 1e-10 * sq
        err = abs(float(got[j] - refld[label][0]))
        guard = abs(got[j] - ref64[label][0]) / float(ref64[label][1])
        print(f"{tag} {label}: {got[j]!r}, err / bound = {err / bound:.3g} (bound {bound:.3g}: solve {solve:.3g}, contract "
              f"{contract:.3g}, 8 x |float64 - longdouble| {other_order:.3g}), S_q {sq:.3g}, |got - float64 helper| / S_q = {guard:.3g}")
        assert guard <= 1e-6, (tag, label, got[j], ref64[label])
        assert err <= bound, (tag, label, got[j], float(refld[label][0]), err, bound)
        worst = max(worst, err / bound)
    return worst


def expected_sources(em):
    """Brute-force restatement of the label -> (order, slot) map: a unit's gradient row holds its order's thawed mean-flux
    labels in label order (Rv left out), then all covariance slots of the order's descriptor: log_amp, log_ls of the global
    kernel if it has one, then mu, log_amp, log_sigma per local kernel."""
    def slot(model, key):
        mean = [k for k in model.labels if not k.startswith(("global_cov:", "local_cov:")) and k != "Rv"]
        if key in mean:
            return mean.index(key)
        base = len(mean)
        if key.startswith("global_cov:"):
            return base + ("log_amp", "log_ls").index(key.split(":")[1])
        _, k, leaf = key.split(":")
        first_local = 2 if "global_cov" in model.params else 0
        return base + first_local + 3 * int(k) + ("mu", "log_amp", "log_sigma").index(leaf)

    out = []
    for label in em.labels:
        if label.startswith("order") and ":" in label and label.split(":", 1)[0][5:].isdigit():
            i, key = int(label.split(":", 1)[0][5:]), label.split(":", 1)[1]
            out.append([(i, slot(em.orders[i], key))])
        elif label == "Rv":
            out.append([])
        else:
            out.append([(i, slot(m, label)) for i, m in enumerate(em.orders) if label in m.labels])
    return out


def reduce_restated(lnl, info, grads, sources):
    """The rule of sf_multi_grad_reduce as a plain loop: lnl, info (n_orders, W), grads[i] (W, stride)."""
    n, W = lnl.shape
    out_l, out_i, out_g = np.empty(W), np.zeros(W, dtype=np.int32), np.zeros((W, len(sources)))
    for w in range(W):
        s = lnl[0, w]
        for i in range(1, n):
            s = s + lnl[i, w]
        code = 0
        for i in range(n):
            if code == 0:
                code = int(info[i, w])
        for j, src in enumerate(sources):
            g = 0.0
            for q, (i, slot) in enumerate(src):
                g = grads[i][w, slot] if q == 0 else g + grads[i][w, slot]
            out_g[w, j] = g
        out_l[w], out_i[w] = s, code
        if code != 0:
            out_l[w] = -np.inf
            out_g[w] = np.nan
    return out_l, out_g, out_i


__all__ = ["CASES", "PER", "build", "oracle_params", "kink_distances", "check_cov_slots", "check_mean_slots", "expected_sources",
           "reduce_restated"]
