"""Multi-order models whose orders sample their own nuisance parameters: every order has its own Chebyshev terms,
log_scale, global kernel and 0, 1 or 3 local kernels (so the C-ABI rows of the orders differ in stride)."""
import numpy as np

from starfish_amd import synth

PER = ("cheb", "log_scale", "global_cov", "local_cov")
SHARED = ("vz", "vsini", "T", "logg", "Z")


def per_order_models(n_local=(0, 1, 3), sizes=None, m=2, seed0=100, no_vsini=()):
    """(orders, models): order i has ``sizes[i]`` pixels (default 64 each) and ``n_local[i]`` local kernels; the
    orders listed in ``no_vsini`` are not broadened."""
    sizes = sizes or [64] * len(n_local)
    orders = [synth.make_order(N=n, m=m, seed=seed0 + i, wave0=5000.0 * 1.02**i) for i, n in enumerate(sizes)]
    models = []
    for i, (o, nl) in enumerate(zip(orders, n_local)):
        c = dict(synth.centre_params(o))
        w, N = o["wave"], len(o["wave"])
        c["local_cov"] = [dict(mu=float(w[(k + 1) * N // (nl + 1)]), log_amp=-8.0 - 0.1 * k, log_sigma=float(np.log(12.0)))
                          for k in range(nl)]
        if not nl:
            del c["local_cov"]
        c["cheb"] = [0.01 * (i + 1), -0.02]
        c["log_scale"] = 0.1 * i
        c["global_cov"] = dict(log_amp=-9.0 + 0.1 * i, log_ls=float(np.log(10.0)))
        if i in no_vsini:
            del c["vsini"]
        models.append(synth.build_model(o, params=c))
    return orders, models


def expected_labels(models):
    out = list(SHARED)
    for i, m in enumerate(models):
        out += [f"order{i}:{k}" for k in m.labels if k.split(":")[0] in PER]
    return tuple(out)


def ball_scale(label):
    """Walker scatter of a (possibly prefixed) label: synth's ball, every local kernel like kernel 0."""
    key = label.split(":", 1)[1] if label.startswith("order") else label
    if key.startswith("local_cov:"):
        key = "local_cov:0:" + key.split(":")[2]
    return synth._BALL[key]


def ball(em, B, seed=1):
    rng = np.random.default_rng(seed)
    p0 = em.get_param_vector()
    scales = np.array([ball_scale(k) for k in em.labels])
    return p0[None, :] + scales[None, :] * rng.standard_normal((B, len(p0)))


def oracle_params(model, vec):
    """One order's own label vector -> oracle.sf_oracle parameter dict."""
    v = dict(zip(model.labels, vec))
    n_local = sum(k.endswith(":mu") for k in v)
    q = dict(vz=v["vz"], log_scale=v["log_scale"], global_cov=(v["global_cov:log_amp"], v["global_cov:log_ls"]),
             cheb=[v["cheb:1"], v["cheb:2"]], grid=[v["T"], v["logg"], v["Z"]])
    if "vsini" in v:
        q["vsini"] = v["vsini"]
    if n_local:
        q["local_cov"] = [(v[f"local_cov:{k}:mu"], v[f"local_cov:{k}:log_amp"], v[f"local_cov:{k}:log_sigma"])
                          for k in range(n_local)]
    return q
