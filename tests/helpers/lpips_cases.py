"""The cases of the LPIPS parity tests (test_lpips_cpu.py, test_lpips_gpu.py) and the recorded distance between the two
modes of helpers/lpips_oracle.py on them.

    python tests/helpers/lpips_cases.py --record     # writes profiles/lpips_parity_margins.json, on the CPU

Per case and layer the file holds the largest absolute error of the float32 chain mode against the float64 mode, for the
feature map (over both images) and for the distance map d, each with max |float64 value|.  The GPU bounds are 2.5 x
these errors.  A ``gpu_used`` section, written from a GPU run, is carried over by ``--record``.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lpips_oracle as orc  # noqa: E402

MARGINS_PATH = os.path.join(ROOT, "profiles", "lpips_parity_margins.json")
WEIGHT_SEED = 17
MARGIN = 2.5  # over a recorded float32-vs-float64 difference, as in test_poisson_cpu.py
# name -> (F, H, W): the smallest frame (f3..f5 are 1 x 1, every tap row meets padding); odd sizes with remainder tiles;
# a wide, flat frame
CASES = {"31x31": (1, 31, 31), "67x95": (3, 67, 95), "35x127": (2, 35, 127)}
_cache = {}


def weights() -> dict:
    from nerf_vo_amd.lpips import synthetic_weights

    if "weights" not in _cache:
        _cache["weights"] = synthetic_weights(WEIGHT_SEED)
    return _cache["weights"]


def frames(name: str) -> tuple:
    """Two uint8 [F, H, W, 3] batches: the second is the first plus uniform noise in +-40, clamped."""
    F, H, W = CASES[name]
    rng = np.random.default_rng(1000 + sorted(CASES).index(name))
    a = rng.integers(0, 256, (F, H, W, 3), dtype=np.int64)
    b = np.clip(a + rng.integers(-40, 41, a.shape), 0, 255)
    return a.astype(np.uint8), b.astype(np.uint8)


def reference(name: str) -> dict:
    """The float64 oracle of a case, computed once per process and shared; do not modify."""
    if name not in _cache:
        a, b = frames(name)
        _cache[name] = orc.lpips(orc.image_of_uint8(a), orc.image_of_uint8(b), weights(), "float64")
    return _cache[name]


def measure(name: str) -> list:
    """Per layer: the chain mode's errors against float64 on this case."""
    a, b = frames(name)
    ref = reference(name)
    chain = orc.lpips(orc.image_of_uint8(a), orc.image_of_uint8(b), weights(), "chain")
    rows = []
    for l in range(5):
        feat_err = max(float((c.double() - r).abs().max()) for c, r in zip(chain["features"][l], ref["features"][l]))
        feat_ref = max(float(r.abs().max()) for r in ref["features"][l])
        rows.append({"feature_err": feat_err, "feature_ref": feat_ref,
                     "map_err": float((chain["maps"][l].double() - ref["maps"][l]).abs().max()),
                     "map_ref": float(ref["maps"][l].abs().max())})
    return rows


def recorded() -> dict:
    with open(MARGINS_PATH) as fh:
        return json.load(fh)


def record() -> None:
    out = {"what": "max abs error of the float32 sequential-chain oracle against the float64 oracle, per case and layer "
                   "(tests/helpers/lpips_cases.py --record); GPU bounds are 2.5 x these",
           "weight_seed": WEIGHT_SEED, "cases": {name: measure(name) for name in CASES}}
    if os.path.exists(MARGINS_PATH):
        old = recorded()
        if "gpu_used" in old:
            out["gpu_used"] = old["gpu_used"]
    with open(MARGINS_PATH, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    for name, rows in out["cases"].items():
        for l, r in enumerate(rows):
            print(f"{name} f{l + 1}: feature {r['feature_err']:.3e} of {r['feature_ref']:.3e} ({r['feature_err'] / r['feature_ref']:.2e}), "
                  f"map {r['map_err']:.3e} of {r['map_ref']:.3e}")


if __name__ == "__main__":
    if "--record" in sys.argv:
        record()
    else:
        print(__doc__)
