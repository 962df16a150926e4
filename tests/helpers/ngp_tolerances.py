"""The float32 error of the occupancy-grid kernel oracle itself, measured on the CPU: every tests/helpers/ngp_oracle.py
reference run in float32 (exponentials as exp2(log2e * x), the way the device's __expf evaluates them) against its float64
run on the same inputs (e32, max|err| / max|ref| per comparison).  The bounds of tests/test_ngp_kernels_gpu.py are
factor * e32 + 1e-6 with these figures.

  python tests/helpers/ngp_tolerances.py                      print the figures (and the largest |x| fed to an exponential)
  python tests/helpers/ngp_tolerances.py --write              rewrite the "e32" / "max_abs_x" blocks of profiles/ngp_parity_margins.json
  python tests/helpers/ngp_tolerances.py --measured FILE      copy the kernel figures a GPU run of the test file recorded
                                                              (NVO_NGP_MEASURED=FILE) into its "measured_gfx950" block
  python tests/helpers/ngp_tolerances.py --table              the EXPERIMENTS.md table of the committed file
"""
import json
import os
import sys

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [TESTS, os.path.dirname(TESTS)]

from helpers import ngp_oracle as N  # noqa: E402


def _load():
    if os.path.exists(N.MARGINS_PATH):
        return N.load_margins()
    return {"rule": "bound = factor * e32 + 1e-6 on the figure; factor 4 unless listed under factors.  d_y (d_rgb_out, stored "
                    "as fp16) is judged ELEMENTWISE: |got - ref| <= bound * max|ref| + half an fp16 ulp of the reference "
                    "(2^-11 |ref| for normal values, 2^-25 absolute in the subnormal range); its recorded figure is "
                    "max over the elements of (|got - ref| - that half ulp, not below 0) / max|ref|",
            "figure": "max|got - ref64| / max|ref64| per comparison",
            "e32_exponential": "float32 runs evaluate exp(x) as exp2(fl32(0x1.715476p+0 * x)), the device's __expf",
            "factors": {}, "e32": {}, "max_abs_x": {}, "measured_gfx950": {}}


def _save(m):
    with open(N.MARGINS_PATH, "w") as fh:
        json.dump(m, fh, indent=1)
        fh.write("\n")


def family(key):
    head, _, q = key.partition(":")
    return head.split("/")[0] + (":" + q if head.startswith("composite/") or q.endswith("_capped") else "")


def table(m):
    fam = {}
    for key, e32 in m["e32"].items():
        got = m["measured_gfx950"].get(key)
        bound = N.bound_for(key, m)
        row = fam.setdefault(family(key), {"n": 0, "e32": 0.0, "got": None, "ratio": 0.0, "worst": "", "x": 0.0})
        row["n"] += 1
        row["e32"] = max(row["e32"], e32)
        row["x"] = max(row["x"], m.get("max_abs_x", {}).get(key, 0.0))
        if got is not None:
            row["got"] = max(row["got"] or 0.0, got)
            if got / bound >= row["ratio"]:
                row["ratio"], row["worst"] = got / bound, key
    print("| family | comparisons | largest abs(x) into exp | largest e32 | largest kernel figure | largest figure / bound | at |")
    print("|---|---|---|---|---|---|---|")
    for name, r in fam.items():
        got = "not measured" if r["got"] is None else f"{r['got']:.2e}"
        ratio = "-" if r["got"] is None else f"{r['ratio']:.2f}"
        print(f"| {name} | {r['n']} | {r['x']:.4g} | {r['e32']:.2e} | {got} | {ratio} | `{r['worst']}` |")


def main():
    m = _load()
    if "--table" in sys.argv:
        return table(m)
    if "--measured" in sys.argv:
        with open(sys.argv[sys.argv.index("--measured") + 1]) as fh:
            m["measured_gfx950"] = json.load(fh)
        return _save(m)
    e32, xs = N.e32_figures(with_x=True)
    for key, v in e32.items():
        print(f"{key:48s} {v:.3e}   |x| <= {xs.get(key, 0.0):.4g}")
    if "--write" in sys.argv:
        m["e32"] = e32
        m["max_abs_x"] = xs
        # (derived, not measured: tests/helpers/ngp_oracle.py CAPPED_FACTOR; entries added by hand stay)
        m["factors"] = {**{k: v for k, v in m.get("factors", {}).items() if k in e32}, **N.derived_factors(e32)}
        _save(m)


if __name__ == "__main__":
    main()
