"""What float32 alone changes in the dense bundle adjustment, measured on the CPU: the oracle's float32 rendering
(helpers/dense_ba_oracle.py with dt=float32: per-pixel terms, per-pixel sums, Q and the depth step in float32; block sums,
Schur complement, solve, retraction and covariance sums in float64, as on the device) against its float64 run, on the
cases of helpers/dense_ba_cases.py.  Figure: max|f32 - f64| / max|f64| per quantity, the largest over the shapes and
window sizes of a family (fixed2 / prior x plain / behind, and the large-P chain).  tests/test_dense_ba_gpu.py records
these figures and bounds every comparison by 4 x the figure.

  python tests/helpers/dense_ba_tolerances.py        print the table as the Python literal the test file holds
"""
import os
import sys

import numpy as np

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [TESTS, os.path.dirname(TESTS)]

from helpers import dense_ba_cases as cases  # noqa: E402
from helpers import dense_ba_oracle as orc  # noqa: E402

FIRST = ("B", "v", "C", "wz", "Ei", "Ej", "S", "g", "dx")   # of the first linearisation
QUANTITIES = ("coords",) + FIRST + ("poses", "disps", "cov_reference", "cov_marginal")


def family(name: str) -> str:
    return "largeP" if "chain" in name else "-".join(name.split("-")[2:])


def figure(got, ref) -> float:
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


def quantities(case, run, dt=np.float64):
    """name -> array of one oracle run (or of anything shaped like it)."""
    first = run["its"][0]
    out = {k: first[k] for k in FIRST}
    out["coords"] = orc.reproject(case["poses"], case["disps"], case["intrinsics"], case["ii"], case["jj"], dt)[0]
    out["poses"], out["disps"] = run["poses"], run["disps"][run["kx"]]
    out["cov_reference"], out["cov_marginal"] = run["cov"]["reference"], run["cov"]["marginal"]
    return out


def e32_figures():
    fig = {}
    for name, kw in cases.grid() + [cases.LARGE_P]:
        case, ref = cases.oracle(name, kw)
        _, low = cases.oracle(name, kw, dt=np.float32)
        a, b = quantities(case, low, np.float32), quantities(case, ref)
        row = fig.setdefault(family(name), {})
        for q in QUANTITIES:
            row[q] = max(row.get(q, 0.0), figure(a[q], b[q]))
    return fig


if __name__ == "__main__":
    fig = e32_figures()
    print("E32 = {")
    for fam, row in fig.items():
        print(f'    "{fam}": {{' + ", ".join(f'"{q}": {v:.2e}' for q, v in row.items()) + "},")
    print("}")
