"""The float32 error of the pose-chain oracle itself, measured on the CPU: every tests/helpers/pose_oracle.py reference
run in float32 against its float64 run on the same inputs (e32, max|err| / max|ref| per comparison).  The bounds of
tests/test_pose_chain_gpu.py are factor * e32 + 1e-6 with these figures.

  python tests/helpers/pose_tolerances.py                      print the figures
  python tests/helpers/pose_tolerances.py --write              rewrite the "e32" block of profiles/pose_parity_margins.json
  python tests/helpers/pose_tolerances.py --measured FILE      copy the kernel figures a GPU run of the test file recorded
                                                               (NVO_POSE_MEASURED=FILE) into its "measured_gfx950" block
  python tests/helpers/pose_tolerances.py --table              the EXPERIMENTS.md table of the committed file
"""
import json
import os
import sys

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [TESTS, os.path.dirname(TESTS)]

from helpers import pose_oracle as P  # noqa: E402


def _load():
    if os.path.exists(P.MARGINS_PATH):
        return P.load_margins()
    return {"rule": "bound = factor * e32 + 1e-6; factor 4 unless listed under factors",
            "figure": "max|got - ref64| / max|ref64| per comparison (per |w| bucket for the exp-map cases)",
            "factors": {}, "e32": {}, "measured_gfx950": {}}


def _save(m):
    with open(P.MARGINS_PATH, "w") as fh:
        json.dump(m, fh, indent=1)
        fh.write("\n")


def table(m):
    fam = {}
    for key, e32 in m["e32"].items():
        name = key.split("/")[0]
        got = m["measured_gfx950"].get(key)
        bound = P.bound_for(key, m)
        row = fam.setdefault(name, {"n": 0, "e32": 0.0, "got": 0.0, "ratio": 0.0, "worst": ""})
        row["n"] += 1
        row["e32"] = max(row["e32"], e32)
        if got is not None:
            row["got"] = max(row["got"], got)
            if got / bound >= row["ratio"]:
                row["ratio"], row["worst"] = got / bound, key
    print("| family | comparisons | largest e32 | largest kernel figure | largest figure / bound | at |")
    print("|---|---|---|---|---|---|")
    for name, r in fam.items():
        print(f"| {name} | {r['n']} | {r['e32']:.2e} | {r['got']:.2e} | {r['ratio']:.2f} | `{r['worst']}` |")
    print()
    print("| exp-map bucket (pen-dev) | SE3 e32 | SE3 kernel | SE3 bound | SO3xR3 e32 | SO3xR3 kernel | SO3xR3 bound |")
    print("|---|---|---|---|---|---|---|")
    for w in P.EXP_BUCKETS["SE3"]:
        cells = []
        for mode in ("SE3", "SO3xR3"):
            key = f"exp/{mode}-pen-dev:w{w:g}"
            if key in m["e32"]:
                got = m["measured_gfx950"].get(key)
                cells += [f"{m['e32'][key]:.2e}", "-" if got is None else f"{got:.2e}", f"{P.bound_for(key, m):.2e}"]
            else:
                cells += ["-", "-", "-"]
        print(f"| {w:g} | " + " | ".join(cells) + " |")


def main():
    m = _load()
    if "--table" in sys.argv:
        return table(m)
    if "--measured" in sys.argv:
        with open(sys.argv[sys.argv.index("--measured") + 1]) as fh:
            m["measured_gfx950"] = json.load(fh)
        return _save(m)
    e32 = P.e32_figures()
    for key, v in e32.items():
        print(f"{key:48s} {v:.3e}")
    if "--write" in sys.argv:
        m["e32"] = e32
        _save(m)


if __name__ == "__main__":
    main()
