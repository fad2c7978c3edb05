"""Inputs and restatements of the multi-order Fisher tests (sf_fisher_banded_multi_batch_md, sf_multi_fisher_reduce,
EchelleModel.fisher_information), on top of tests/echelle_banded_cases.py (EB).  Nothing here touches a device.

Cases A, B, C and C-wide: EB.build's (8 mean columns per order; m = 2, 4, 4: 11, 13, 13 rows of the sweep).
Case D: case A with order 1 given four Chebyshev coefficients -- 10 columns beside 8, 13 rows: orders 0 and 2 carry two zero
rows behind their own columns.
Case E: case B with every order at six Chebyshev coefficients -- 1 + 4 + 12 = 17 rows, the second 16-row block of right-hand
sides: the window is 128, the bounds stay those of case B (at most 126).
D and E with three walkers drawn as per_order_cases.ball draws them (seed 1), the further coefficients scattered like cheb:1."""
import re

import numpy as np

from per_order_cases import PER, ball_scale
from starfish_amd import synth
from starfish_amd.models import EchelleModel

import echelle_banded_cases as EB
import echelle_gradient_cases as EG

CHEB = (0.01, -0.02, 0.004, -0.003, 0.002, -0.001)  # (the further terms: those of tests/test_gpu_fisher.py's N180-c6)
ROWS = {"A": 11, "B": 13, "C": 13, "D": 13, "E": 17}  # 1 + m + the largest column count of an order
COLUMNS = {"A": (8, 8, 8), "B": (8, 8, 8), "C": (8, 8, 8), "D": (8, 10, 8), "E": (12, 12, 12)}
WINDOWS = {11: 144, 13: 144, 17: 128}  # sf_band_max_halfwidth at that row count
CASES = ("A", "B", "C", "D", "E")
_PREFIXED = re.compile(r"order(\d+):(.+)$")


def models_with_cheb(n_local, sizes, m, n_cheb, seed0=100):
    """per_order_cases.per_order_models with ``n_cheb[i]`` Chebyshev coefficients in order i (its first two are that builder's)."""
    orders = [synth.make_order(N=n, m=m, seed=seed0 + i, wave0=5000.0 * 1.02**i) for i, n in enumerate(sizes)]
    models = []
    for i, (o, nl, nc) in enumerate(zip(orders, n_local, n_cheb)):
        c = dict(synth.centre_params(o))
        w, N = o["wave"], len(o["wave"])
        c["local_cov"] = [dict(mu=float(w[(k + 1) * N // (nl + 1)]), log_amp=-8.0 - 0.1 * k, log_sigma=float(np.log(12.0)))
                          for k in range(nl)]
        if not nl:
            del c["local_cov"]
        c["cheb"] = [0.01 * (i + 1), *CHEB[1:nc]]
        c["log_scale"] = 0.1 * i
        c["global_cov"] = dict(log_amp=-9.0 + 0.1 * i, log_ls=float(np.log(10.0)))
        models.append(synth.build_model(o, params=c))
    return orders, models


def ball(em, B, seed=1):
    rng = np.random.default_rng(seed)
    p0 = em.get_param_vector()
    scales = np.array([1e-3 if ":cheb:" in f":{k}" else ball_scale(k) for k in em.labels])
    return p0[None, :] + scales[None, :] * rng.standard_normal((B, len(p0)))


def build(name):
    """(orders, models, em, P) of case A, B, C, "C-wide", D or E."""
    if name in ("A", "B", "C", "C-wide"):
        return EB.build(name)
    n_local, sizes, m, _ = EG.CASES["A" if name == "D" else "B"]
    orders, models = models_with_cheb(n_local, sizes, m, (2, 4, 2) if name == "D" else (6, 6, 6))
    em = EchelleModel.from_orders(models, per_order=PER)
    return orders, models, em, ball(em, 3, seed=1)


def is_mean(key):
    return not key.startswith(("global_cov:", "local_cov:")) and key != "Rv"


def expected_mean_labels(em):
    out = []
    for label in em.labels:
        hit = _PREFIXED.match(label)
        if is_mean(hit.group(2) if hit else label):
            out.append(label)
    return tuple(out)


def expected_sources(em):
    """Brute-force restatement of the label -> (order, slot) map of the Fisher matrix: a unit's matrix is in its order's thawed
    mean-flux labels in label order (covariance labels and Rv left out)."""
    mean = [[k for k in m.labels if is_mean(k)] for m in em.orders]
    out = []
    for label in expected_mean_labels(em):
        hit = _PREFIXED.match(label)
        if hit:
            i = int(hit.group(1))
            out.append([(i, mean[i].index(hit.group(2)))])
        else:
            out.append([(i, mine.index(label)) for i, mine in enumerate(mean) if label in mine])
    return out


def oracle_params(model, vec):
    """One order's own label vector -> oracle.sf_oracle parameter dict, with however many Chebyshev coefficients it has."""
    v = dict(zip(model.labels, vec))
    n_local = sum(k.endswith(":mu") for k in v)
    n_cheb = sum(k.startswith("cheb:") for k in v)
    q = dict(vz=v["vz"], vsini=v["vsini"], log_scale=v["log_scale"], global_cov=(v["global_cov:log_amp"], v["global_cov:log_ls"]),
             cheb=[v[f"cheb:{k}"] for k in range(1, n_cheb + 1)], grid=[v["T"], v["logg"], v["Z"]])
    if n_local:
        q["local_cov"] = [(v[f"local_cov:{k}:mu"], v[f"local_cov:{k}:log_amp"], v[f"local_cov:{k}:log_sigma"])
                          for k in range(n_local)]
    return q


def reduce_restated(lnl, info, fishers, sources):
    """The rule of sf_multi_fisher_reduce as a plain loop: lnl, info (n_orders, W), fishers[i] (W, p_i, p_i)."""
    n, W = lnl.shape
    p = len(sources)
    out_l, out_i, out_f = np.empty(W), np.zeros(W, dtype=np.int32), np.zeros((W, p, p))
    for w in range(W):
        s = lnl[0, w]
        for i in range(1, n):
            s = s + lnl[i, w]
        code = 0
        for i in range(n):
            if code == 0:
                code = int(info[i, w])
        for a in range(p):
            for b in range(a + 1):
                slot_b = dict(sources[b])
                f, first = 0.0, True
                for i, slot_a in sorted(sources[a]):
                    if i in slot_b:
                        term = fishers[i][w, slot_a, slot_b[i]]
                        f = term if first else f + term
                        first = False
                out_f[w, a, b] = out_f[w, b, a] = f
        out_l[w], out_i[w] = s, code
        if code != 0:
            out_l[w] = -np.inf
            out_f[w] = np.nan
    return out_l, out_f, out_i
