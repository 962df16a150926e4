"""The float32 error of the optimiser oracle itself, measured on the CPU: every comparison of
tests/test_optimizer_kernels_gpu.py with tests/helpers/adam_oracle.py run in float32 against its float64 run on the same
inputs (e32 = max|f32 - f64| / max|f64| per comparison key).  The bound of a comparison is 4 x e32, without a floor: a
quantity whose e32 is exactly zero is compared for equality.  Quantities: the update p_after - p_before (formed in float64
from the two fp32 buffers), m, v and the weight average.

  python tests/helpers/adam_tolerances.py                      print e32 per comparison key
  python tests/helpers/adam_tolerances.py --write              rewrite the "e32" block of profiles/adam_parity_margins.json
  python tests/helpers/adam_tolerances.py --measured FILE      copy the figures a GPU run of the test file recorded
                                                               (NVO_ADAM_MEASURED=FILE) into "measured_gfx950" / "records"
  python tests/helpers/adam_tolerances.py --table              the EXPERIMENTS.md table of the committed file
"""
import json
import os
import sys

import numpy as np

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [TESTS, os.path.dirname(TESTS)]

from helpers import adam_cases as cases  # noqa: E402
from helpers import adam_oracle as A  # noqa: E402

F32, F64 = np.float32, np.float64
_cache = {}


def quantities(p_before, st, ema=None):
    """the judged quantities of one run: the update in float64 from the two buffers, the moments, the average"""
    out = {"update": np.asarray(st["p"], F64) - np.asarray(p_before, F64), "m": np.asarray(st["m"], F64),
           "v": np.asarray(st["v"], F64)}
    if ema is not None:
        out["ema"] = np.asarray(ema, F64)
    return out


def run_step(c, dtype):
    """one launch of a case through the oracle (with the weight average of the stepped groups where the case has one)"""
    args = cases.args_of(c)
    st = A.adam_step(c["state"], c["grads"], c["groups"], args, dtype)
    ema = None
    if c["ema"] is not None:
        ema = c["ema"]["values"].astype(dtype)
        for g in c["groups"]:
            if g["n"] and not (c["flags"] is not None and c["flags"][g["slot"]]):
                s = slice(g["offset"], g["offset"] + g["n"])
                ema[s] = A.ema_update(ema[s], st["p"][s], c["ema"]["decay"], c["ema"]["t0"] + 1, dtype)
    return quantities(c["state"]["p"], st, ema)


def _builders():
    """comparison family -> builder of (case, float64 quantities, float32 quantities); keys are family:quantity"""
    b = {}
    for name in cases.STEP_CASES:
        b[f"step/{name}"] = lambda name=name: cases.step_case(name)
    b["cap"] = cases.cap_case
    for name in cases.TAIL_CASES:
        b[f"tail/{name}"] = lambda name=name: cases.tail_case(name)
    return b


BUILDERS = _builders()


def reference(family):
    """(case, float64 quantities) of a step family, computed once per process"""
    if family not in _cache:
        c = BUILDERS[family]()
        _cache[family] = (c, run_step(c, F64))
    return _cache[family]


def trajectory_reference():
    if "trajectory" not in _cache:
        c = cases.trajectory_case()
        st, cs = cases.trajectory_oracle(c, F64)
        _cache["trajectory"] = (c, quantities(c["state"]["p"], st), cs)
    return _cache["trajectory"]


def ema_reference(decay, t0, shift, dtype=F64):
    c = cases.ema_case(decay, t0, shift)
    return c, A.ema_update(c["ema"], c["p"], decay, t0 + 1, dtype)


def e32_figures():
    fig = {}
    for family in BUILDERS:
        c, ref = reference(family)
        low = run_step(c, F32)
        for q in ref:
            fig[f"{family}:{q}"] = A.figure(low[q], ref[q])
        if family == "cap":
            _cache.pop(family)   # (the one large case: not kept)
    c, ref, _ = trajectory_reference()
    st32, _ = cases.trajectory_oracle(c, F32)
    low = quantities(c["state"]["p"], st32)
    for q in ref:
        fig[f"trajectory:{q}"] = A.figure(low[q], ref[q])
    for d, t0, s in cases.EMA_GRID:
        _, ref = ema_reference(d, t0, s)
        _, low = ema_reference(d, t0, s, F32)
        fig[cases.ema_key(d, t0, s)] = A.figure(low, ref)
    return fig


def _load():
    if os.path.exists(A.MARGINS_PATH):
        return A.load_margins()
    return {"rule": "bound = 4 x e32 on the figure, no floor; a quantity whose e32 is exactly zero is compared for equality",
            "figure": "max|got - ref64| / max|ref64| per quantity and case; update = p_after - p_before in float64",
            "e32": {}, "measured_gfx950": {}, "records": {}}


def _save(m):
    with open(A.MARGINS_PATH, "w") as fh:
        json.dump(m, fh, indent=1)
        fh.write("\n")


def table(m):
    fam = {}
    for key, e32 in m["e32"].items():
        head, _, q = key.partition(":")
        name = head.split("/")[0] + ("/" + head.split("/")[1].split("-")[0] if head.startswith("step/") else "") + ":" + q
        got = m["measured_gfx950"].get(key)
        bound = A.bound_for(key, m)
        row = fam.setdefault(name, {"n": 0, "e32": 0.0, "got": None, "ratio": 0.0, "worst": ""})
        row["n"] += 1
        row["e32"] = max(row["e32"], e32)
        if got is not None:
            row["got"] = max(row["got"] or 0.0, got)
            ratio = got / bound if bound > 0.0 else (0.0 if got == 0.0 else float("inf"))
            if ratio >= row["ratio"]:
                row["ratio"], row["worst"] = ratio, key
    print("| family | comparisons | largest e32 | largest kernel figure | largest figure / bound | at |")
    print("|---|---|---|---|---|---|")
    for name, r in fam.items():
        got = "not measured" if r["got"] is None else f"{r['got']:.2e}"
        ratio = "-" if r["got"] is None else f"{r['ratio']:.2f}"
        print(f"| {name} | {r['n']} | {r['e32']:.2e} | {got} | {ratio} | `{r['worst']}` |")


def main():
    m = _load()
    if "--table" in sys.argv:
        return table(m)
    if "--measured" in sys.argv:
        with open(sys.argv[sys.argv.index("--measured") + 1]) as fh:
            got = json.load(fh)
        m["measured_gfx950"] = got.get("figures", {})
        m["records"] = got.get("records", {})
        return _save(m)
    e32 = e32_figures()
    for key, v in e32.items():
        print(f"{key:40s} {v:.3e}")
    if "--write" in sys.argv:
        m["e32"] = e32
        _save(m)


if __name__ == "__main__":
    main()
