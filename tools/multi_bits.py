"""Bit comparison of everything the multi-order calls return, for refactors of the multi-order host layer (csrc/sf_multi*.cpp)
and of its plans in the Python device layer:
    SF_LIB_PATH=<one build> python tools/multi_bits.py > a.json
    SF_LIB_PATH=<another>   python tools/multi_bits.py > b.json
    python tools/multi_bits.py --compare a.json b.json      -> lists the keys that differ, exit code 1 if any
Prints ONE JSON object {"<case>/<output>": sha256 of the raw bytes returned, "<case>/<fact>": an integer of the plan (calls,
re-routed units, half-width)} for a fixed, seeded list of small cases, three walkers unless said otherwise, so that every branch
of the four entry points runs once:
  likelihood       per_order_models((0, 1, 3), sizes=[64, 130, 180], m=2): one shared descriptor (order 0's rows for every order)
                   and one per order, each whole and with max_units = 4 (a cut inside an order)
  gradient         cases A and B of tests/echelle_gradient_cases.py with their order sum; A with the middle order requesting
                   nothing and max_units = 3 (one piece is a plain likelihood call)
  banded gradient  cases A - C of tests/echelle_banded_cases.py under "banded" and "auto"; C-wide (a unit beyond the window); A with
                   max_units = 4; the order sum on the device (A) and on the host (C-wide under "auto")
  banded Fisher    cases A, D, E of tests/echelle_fisher_cases.py under "banded" and "auto"; A with max_units = 4; the order sum on
                   the device (A) and on the host (C-wide under "auto")
  two chunks       four orders (64, 130, 180, 96 pixels; 0, 1, 3, 1 local kernels) x 100 walkers = 400 units through all four
                   entry points: the first chunk closes behind the third segment (300 >= 256 units), a second chunk exists and
                   lane 0 is used twice
Only names of starfish_amd._device are used.  It hashes results only -- nothing inside a workspace.  Needs an MI355X."""
import hashlib
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np

TWO_CHUNK = dict(n_local=(0, 1, 3, 1), sizes=[64, 130, 180, 96], m=2, walkers=100, seed=2)  # (seed: every unit fits the LDS window)
_BUILT = {}


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def put(out, key, per_order):
    """The per-order dicts of a collected call."""
    for i, res in enumerate(per_order):
        for name, v in res.items():
            out[f"{key}/order{i}.{name}"] = digest(v)


def put_sum(out, key, total, names):
    for name, v in zip(names, total):
        out[f"{key}/sum.{name}"] = digest(v)


def built(module, name):
    """(orders, models, em, P) of ``module.build(name)``, made once."""
    if (module.__name__, name) not in _BUILT:
        _BUILT[module.__name__, name] = module.build(name)
    return _BUILT[module.__name__, name]


def two_chunk_model():
    if "two-chunk" not in _BUILT:
        from per_order_cases import PER, ball, per_order_models
        from starfish_amd.models import EchelleModel

        orders, models = per_order_models(TWO_CHUNK["n_local"], sizes=list(TWO_CHUNK["sizes"]), m=TWO_CHUNK["m"], seed0=100)
        em = EchelleModel.from_orders(models, per_order=PER)
        _BUILT["two-chunk"] = (orders, models, em, ball(em, TWO_CHUNK["walkers"], seed=TWO_CHUNK["seed"]))
    return _BUILT["two-chunk"]


def pack(models, P, cols):
    packed = [m._pack(P[:, cols[i]], update_caches=False) for i, m in enumerate(models)]
    return tuple([p[k] for p in packed] for k in range(3))  # devs, mds, rows


def run_likelihood(out, key, devs, md, rows, **kw):
    from starfish_amd import _device as D

    plan = D.loglike_multi(devs, md, rows, sync=False, **kw)
    out[f"{key}/calls"] = len(plan.calls)
    put(out, key, plan.collect())


def run_gradient(out, key, devs, mds, rows, requests, sources=None, **kw):
    from starfish_amd import _device as D

    plan = D.loglike_multi_grad(devs, mds, rows, requests, sync=False, **kw)
    out[f"{key}/calls"] = len(plan.calls)
    put(out, key, plan.collect())
    if sources is not None:
        put_sum(out, key, plan.reduce(sources), ("lnl", "grad", "info"))


def run_banded(out, key, kind, devs, mds, rows, wanted, sources=None, **kw):
    """kind: "grad" (``wanted``: the requests) or "fisher" (the columns)."""
    from starfish_amd import _device as D

    call = D.loglike_banded_multi_grad if kind == "grad" else D.fisher_banded_multi
    plan = call(devs, mds, rows, wanted, sync=False, **kw)
    res = plan.collect()
    out[f"{key}/calls"] = len(plan.plan.calls) if plan.plan is not None else 0
    out[f"{key}/rerouted"], out[f"{key}/halfwidth"], out[f"{key}/complete"] = int(plan.rerouted), int(plan.halfwidth), int(plan.complete)
    put(out, key, res)
    if sources is not None:
        put_sum(out, key, plan.reduce(sources), ("lnl", kind, "info"))


def likelihood_cases(out):
    from per_order_cases import PER, ball, per_order_models
    from starfish_amd.models import EchelleModel

    _, models = per_order_models((0, 1, 3), sizes=[64, 130, 180], m=2)
    em = EchelleModel.from_orders(models, per_order=PER)
    devs, mds, rows = pack(models, ball(em, 3, seed=1), em._layout()[1])
    for tag, kw in (("", {}), ("-cut4", dict(max_units=4))):
        run_likelihood(out, f"loglike-shared{tag}", devs, mds[0], [rows[0]] * 3, **kw)
        run_likelihood(out, f"loglike-per-order{tag}", devs, mds, rows, **kw)


def gradient_cases(out):
    import echelle_gradient_cases as EG

    for name in ("A", "B"):
        _, models, em, P = built(EG, name)
        _, cols, requests, sources = em._gradient_layout()
        devs, mds, rows = pack(models, P, cols)
        run_gradient(out, f"grad-{name}", devs, mds, rows, requests, sources)
        if name == "A":
            run_gradient(out, "grad-A-middle-empty-cut3", devs, mds, rows, [requests[0], ([], False), requests[2]], max_units=3)


def banded_gradient_cases(out):
    import echelle_banded_cases as EB

    for name in ("A", "B", "C", "C-wide"):
        _, models, em, P = built(EB, name)
        _, cols, requests, sources = em._gradient_layout(solver="banded")
        devs, mds, rows = pack(models, P, cols)
        for solver in ("banded", "auto"):
            run_banded(out, f"banded-grad-{name}-{solver}", "grad", devs, mds, rows, requests,
                       sources if name in ("A", "C-wide") else None, solver=solver)
        if name == "A":
            run_banded(out, "banded-grad-A-cut4", "grad", devs, mds, rows, requests, max_units=4)


def banded_fisher_cases(out):
    import echelle_fisher_cases as EF

    for name in ("A", "D", "E", "C-wide"):
        _, models, em, P = built(EF, name)
        _, cols, columns, sources = em._fisher_layout(solver="banded")
        devs, mds, rows = pack(models, P, cols)
        for solver in ("banded", "auto"):
            run_banded(out, f"banded-fisher-{name}-{solver}", "fisher", devs, mds, rows, columns,
                       sources if name in ("A", "C-wide") else None, solver=solver)
        if name == "A":
            run_banded(out, "banded-fisher-A-cut4", "fisher", devs, mds, rows, columns, max_units=4)


def two_chunk_cases(out):
    _, models, em, P = two_chunk_model()
    _, cols, requests, sources = em._gradient_layout(solver="banded")
    devs, mds, rows = pack(models, P, cols)
    run_likelihood(out, "two-chunk-loglike", devs, mds, rows)
    run_gradient(out, "two-chunk-grad", devs, mds, rows, requests, sources)
    run_banded(out, "two-chunk-banded-grad", "grad", devs, mds, rows, requests, sources)
    _, cols, columns, sources = em._fisher_layout(solver="banded")
    run_banded(out, "two-chunk-banded-fisher", "fisher", devs, mds, rows, columns, sources)


GROUPS = {"likelihood": likelihood_cases, "gradient": gradient_cases, "banded-gradient": banded_gradient_cases,
          "banded-fisher": banded_fisher_cases, "two-chunk": two_chunk_cases}


def main():
    out = {}
    for group, run in GROUPS.items():
        got = {}
        run(got)
        out.update({f"{group}:{k}": v for k, v in got.items()})
    print(json.dumps(out, sort_keys=True))


def compare(path_a, path_b):
    def load(path):  # the tool's output (its last line, behind whatever a run printed before it) or the indented fixture
        text = open(path).read().strip()
        return json.loads(text if text.startswith("{") else text.splitlines()[-1])

    a, b = load(path_a), load(path_b)
    bad = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    for k in bad:
        print("DIFFERS:", k)
    print(f"{len(a)} / {len(b)} entries, {len(bad)} differ")
    return 1 if bad or not a else 0


if __name__ == "__main__":
    sys.exit(compare(*sys.argv[2:4]) if sys.argv[1:2] == ["--compare"] else main())
