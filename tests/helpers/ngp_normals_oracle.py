"""Plain-torch CPU references of the occupancy-grid back-end's normals path (csrc/ngp.hip: nvo_ngp_composite_normals;
NgpEngine.density_gradient_at) and the seeded cases of tests/test_ngp_normals_gpu.py / tests/test_ngp_normals_cpu.py.

``normals_reference`` takes ``dtype=``: float64 is the reference, the float32 run of the same function the yardstick
(bound = 4 * e32 + 1e-6 on max|got - ref64| / max|ref64|, profiles/ngp_normals_parity_margins.json) -- the pattern of
tests/helpers/ngp_oracle.py, whose generators and weight arithmetic (``_ray_pass``: the colour pass's own) it reuses.

  python tests/helpers/ngp_normals_oracle.py                  print e32 and the class counts
  python tests/helpers/ngp_normals_oracle.py --write          rewrite the "e32" block of the JSON
  python tests/helpers/ngp_normals_oracle.py --measured FILE  copy the figures a GPU run recorded (NVO_NGP_NORMALS_MEASURED=FILE)
                                                              into "measured_gfx950" and set the chain bounds from them
"""
from __future__ import annotations

import json
import math
import os
import sys

import numpy as np
import torch

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if TESTS not in sys.path:
    sys.path[:0] = [TESTS, os.path.dirname(TESTS)]

from helpers import ngp_oracle as N  # noqa: E402

F64, F32 = N.F64, N.F32
MARGINS_PATH = os.path.join(N.ROOT, "profiles", "ngp_normals_parity_margins.json")
FACTOR = N.DEFAULT_FACTOR
FLOOR = N.FLOOR
BOX = (-8.0, 8.0)       # aabb of the kernel-level case: 1 / (hi - lo) = 2^-4 exactly, so a face coordinate is exactly 0 or 1
FACE_MARGIN = 1e-4      # no other sample's normalised coordinate within this of 0 or 1 (the mask must not depend on rounding)
ROUND_CUTS = N.ROUND_CUTS
CHAIN_FACTOR = 2.5      # the project's convention for chain tolerances: bound = 2.5 x the measured value


# ------------------------------------------------------------------------------------------------------------------
# nvo_ngp_composite_normals
# ------------------------------------------------------------------------------------------------------------------
def normals_case(seed=0, specials=False):
    """``ngp_oracle.composite_case`` (rays of 0, 1, 2, 63, 64, 65, 127 .. 200 samples in shuffled order, a ray the pack
    dropped at the capacity -- count 0, its slots kept -- and free slots behind the last offset, NaN in every slot no ray
    owns) with what the normals kernel reads on top: origins / directions in the box ``BOX`` and dx01 [capacity][3].
    Classes: ``face0`` / ``face1`` -- rays that run INSIDE a face of the box (origin exactly on it, no direction component
    across it: the normalised coordinate of every sample is exactly 0 or exactly 1 on that axis, the mask applies);
    ``outside`` -- samples of a ray that leaves the box; ``zero_grad`` -- samples whose dx01 row is exactly zero;
    ``one_axis`` -- samples with a single non-zero component; the others have components of 10^(-3..3).
    ``specials``: the generator's capped / infinite pre-activations (judged apart, ngp_oracle.CAPPED_FACTOR)."""
    case = N.composite_case(seed=seed, specials=specials)
    g = torch.Generator().manual_seed(9100 + seed)
    R, cap = case["R"], case["capacity"]
    lo, hi = BOX
    origins = (torch.rand(R, 3, generator=g) - 0.5) * 2.0
    directions = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    by_n = {}
    for r in range(R):
        by_n.setdefault(int(case["counts"][r]), []).append(r)
    cls = dict(case["classes"])
    # rays inside a face: axis k fixed at lo (ray of 65 samples) and at hi (ray of 64 samples)
    r0, r1 = by_n[65][0], by_n[64][0]
    for r, k, v in ((r0, 1, lo), (r1, 2, hi)):
        origins[r, k] = v
        d = directions[r].clone()
        d[k] = 0.0
        directions[r] = d / d.norm()
    # a ray that leaves the box through the +x face part-way (t runs to ~5: origin 2.47 in front of the face)
    r_out = by_n[200][0]
    origins[r_out] = torch.tensor([hi - 2.47, 0.25, -0.5])
    directions[r_out] = torch.nn.functional.normalize(torch.tensor([1.0, 0.05, -0.1]), dim=0)
    mag = 10.0 ** (torch.rand(cap, 3, generator=g) * 6.0 - 3.0)
    dx01 = torch.randn(cap, 3, generator=g) * mag
    live = case["ray_idx"] >= 0
    pick = torch.rand(cap, generator=g)
    zero = live & (pick < 0.04)
    one = live & (pick >= 0.04) & (pick < 0.08)
    dx01[zero] = 0.0
    keep_axis = torch.randint(0, 3, (cap,), generator=g)
    for k in range(3):
        dx01[one & (keep_axis != k), k] = 0.0
    dx01[~live] = float("nan")
    # class counts: masks in float64 on the float32 inputs
    x = _coords(case, origins, directions, F64)
    on0 = live[:, None] & (x == 0.0)
    on1 = live[:, None] & (x == 1.0)
    outside = live[:, None] & ((x < 0.0) | (x > 1.0))
    near = live[:, None] & ~on0 & ~on1 & (((x - 0.0).abs() < FACE_MARGIN) | ((x - 1.0).abs() < FACE_MARGIN))
    cls.update({"face0": int(on0.any(1).sum()), "face1": int(on1.any(1).sum()), "outside": int(outside.any(1).sum()),
                "near_face": int(near.any(1).sum()), "zero_grad": int(zero.sum()), "one_axis": int(one.sum()),
                "face0_expected": int(case["counts"][r0]), "face1_expected": int(case["counts"][r1])})
    case.update({"origins": origins, "directions": directions, "dx01": dx01, "lo": lo, "hi": hi,
                 "inv": float(np.float32(1.0) / (np.float32(hi) - np.float32(lo))), "classes": cls})
    return case


def _coords(case, origins, directions, dtype):
    """unclamped normalised coordinate of every slot [capacity][3] (NaN where no ray owns the slot)"""
    lo, hi = BOX
    inv = float(np.float32(1.0) / (np.float32(hi) - np.float32(lo)))
    r = case["ray_idx"].long().clamp_min(0)
    t = case["t"].to(dtype)
    w = origins.to(dtype)[r] + directions.to(dtype)[r] * t[:, None]
    return (w - torch.tensor(lo, dtype=dtype)) * torch.tensor(inv, dtype=dtype)


def normals_reference(case, dtype=F64, counts=None, offsets=None, carry_in=None, accumulate=None):
    """The header contract of nvo_ngp_normal_args: per ray S = sum_i w_i n_i with w the colour pass's weights
    (ngp_oracle._ray_pass: sigma = exp(pre), dd = min(sigma dt, 128), T from the inclusive sum plus carry_in,
    w = (1 - exp(-dd)) T), g = dx01 * inv zeroed on an axis whose unclamped coordinate (o + t d - lo) * inv is not strictly
    inside (0, 1), n = -g / (|g| + 1e-10).  ``accumulate`` [R][3]: a later round adds to it.  -> {"S", "capped_ray"}"""
    R = case["R"]
    counts = case["counts"] if counts is None else counts
    offsets = case["offsets"] if offsets is None else offsets
    rec = N._Rec()
    S = torch.zeros(R, 3, dtype=dtype) if accumulate is None else accumulate.to(dtype).clone()
    capped = torch.zeros(R, dtype=torch.bool)
    x_all = _coords(case, case["origins"], case["directions"], dtype)
    inv = torch.tensor(case["inv"], dtype=dtype)
    for r in range(R):
        n, base = int(counts[r]), int(offsets[r])
        if n == 0:
            continue
        sl = slice(base, base + n)
        c_in = torch.zeros((), dtype=dtype) if carry_in is None else carry_in[r].to(dtype)
        _, dd, _, _, w, _ = N._ray_pass(case["pre"][sl], case["y"][sl], case["t"][sl], case["dt"][sl], c_in, dtype, rec)
        x = x_all[sl]
        g = torch.where((x > 0.0) & (x < 1.0), case["dx01"][sl].to(dtype) * inv, torch.zeros((), dtype=dtype))
        nrm = -g / (torch.sqrt((g * g).sum(1, keepdim=True)) + 1e-10)
        S[r] = S[r] + (w[:, None] * nrm).sum(0)
        capped[r] = bool((~(dd < N.DD_CAP)).any())
    return {"S": S, "capped_ray": capped}


def carry_reference(case, counts, offsets, dtype=F64):
    """optical depth each ray has gathered over the given ranges (the colour kernel's carry_out)"""
    return N.composite_reference(case, False, dict(background=False), dtype, counts=counts, offsets=offsets)["carry"]


def e32_figures():
    """{key: e32}: "normals" -- the case of the kernel test (no capped sample), all rays; "specials/normals" and
    "specials/normals_capped" -- the generator's special values, rays with a capped sample apart"""
    out = {}
    case = normals_case()
    r64, r32 = normals_reference(case, F64), normals_reference(case, F32)
    assert not bool(r64["capped_ray"].any())
    out["normals"] = N.figure(r32["S"], r64["S"])
    case = normals_case(specials=True)
    r64, r32 = normals_reference(case, F64), normals_reference(case, F32)
    c = r64["capped_ray"]
    out["specials/normals"] = N.figure(r32["S"][~c], r64["S"][~c])
    out["specials/normals_capped"] = N.figure(r32["S"][c], r64["S"][c])
    return out


def load_margins():
    with open(MARGINS_PATH) as fh:
        return json.load(fh)


def bound_for(key, margins):
    factor = margins.get("factors", {}).get(key, {}).get("factor", FACTOR)
    return factor * margins["e32"][key] + FLOOR


# ------------------------------------------------------------------------------------------------------------------
# NgpEngine.density_gradient_at: float64 autograd through oracle.grid_encode / oracle.mlp_forward, no 16-bit emulation
# ------------------------------------------------------------------------------------------------------------------
GRAD_INSIDE, GRAD_FACE, GRAD_OUTSIDE = 3000, 240, 200
GRAD_MAX_BELOW = 0.05       # at most this share of the inside points may have a reference gradient norm below the floor
GRAD_FLOOR_REL = 1e-3       # floor = this x the median reference gradient norm of the inside points
N_DENSITY_MLP = 64 * 32 + 16 * 64


def gradient_case(n_grid_params, aabb=(-1.5, 2.5), seed=0):
    """Parameters at a scale where the field is not flat (tests/test_ngp_gpu.py::_engine's: density MLP +-0.25, hash grid
    +-0.8) and positions of the engine's normalised frame: GRAD_INSIDE strictly inside the scene box, GRAD_FACE with one
    coordinate exactly on a face (lo or hi, every axis), GRAD_OUTSIDE outside."""
    g = torch.Generator().manual_seed(7700 + seed)
    lo, hi = aabb
    mlp = (torch.rand(N_DENSITY_MLP, generator=g) * 2 - 1) * 0.25
    grid = (torch.rand(n_grid_params, generator=g) * 2 - 1) * 0.8
    inside = lo + (hi - lo) * (0.001 + 0.998 * torch.rand(GRAD_INSIDE, 3, generator=g))
    face = lo + (hi - lo) * (0.001 + 0.998 * torch.rand(GRAD_FACE, 3, generator=g))
    for i in range(GRAD_FACE):
        face[i, i % 3] = lo if (i // 3) % 2 == 0 else hi
    outside = lo + (hi - lo) * torch.rand(GRAD_OUTSIDE, 3, generator=g)
    for i in range(GRAD_OUTSIDE):
        outside[i, i % 3] = (lo - 0.01 - torch.rand(1, generator=g).item()) if (i // 3) % 2 == 0 else (hi + 0.01 + torch.rand(1, generator=g).item())
    pos = torch.cat([inside, face, outside]).float()
    kind = torch.cat([torch.zeros(GRAD_INSIDE), torch.ones(GRAD_FACE), torch.full((GRAD_OUTSIDE,), 2.0)]).long()
    return {"mlp": mlp, "grid": grid, "positions": pos, "kind": kind, "lo": lo, "hi": hi,
            "classes": {"inside": GRAD_INSIDE, "face": GRAD_FACE, "outside": GRAD_OUTSIDE}}


def gradient_reference(case, aabb_scale=4):
    """(density [M], gradient [M, 3]) in float64: density = exp(pre) of the fp16-ROUNDED parameters (what the engine
    holds) evaluated without any 16-bit emulation, gradient = autograd of the density with respect to the normalised
    input, divided by the box size, zero on an axis whose coordinate is not strictly inside the box; zeros outside."""
    from oracle import mlp as M
    from oracle.ngp import NgpOracle

    orc = NgpOracle(aabb_scale=aabb_scale, emulate_fp16=False)
    lo, hi = case["lo"], case["hi"]
    p = case["positions"].double()
    # (the network input as the engine forms it, in float32: the cell a point falls into at the finest levels must be the
    # kernel's own, or the two sides differentiate different trilinear pieces)
    u = ((case["positions"].float() - lo) / (hi - lo)).double()
    x01 = u.clamp(0.0, 1.0).clone().requires_grad_(True)
    table = case["grid"].half().double().view(-1, 2)
    w = M.split_weights(case["mlp"].half().double(), 32, 16, 64, 1)
    from oracle import grid as G

    enc = G.grid_encode(orc.spec, x01, table, quantize_output=False)
    pre = M.mlp_forward(enc, w, "ReLU", "None", pad_value=0.0, emulate_fp16=False)[:, 0]
    dens = torch.exp(pre)
    dens.sum().backward()
    inside = ((p >= lo) & (p <= hi)).all(1)
    grad = x01.grad / (hi - lo)
    grad = torch.where((u > 0.0) & (u < 1.0) & inside[:, None], grad, torch.zeros((), dtype=F64))
    return torch.where(inside, dens.detach(), torch.zeros((), dtype=F64)), grad


def gradient_floor(ref_grad, kind):
    norm = ref_grad.norm(dim=1)
    floor = GRAD_FLOOR_REL * float(norm[kind == 0].median())
    share = float((norm[kind == 0] < floor).double().mean())
    return floor, share


def angles_deg(a, b):
    a, b = a.double(), b.double()
    c = (a * b).sum(1) / (a.norm(dim=1) * b.norm(dim=1)).clamp_min(1e-300)
    return torch.rad2deg(torch.acos(c.clamp(-1.0, 1.0)))


# ------------------------------------------------------------------------------------------------------------------
def _load_or_new():
    if os.path.exists(MARGINS_PATH):
        return load_margins()
    return {"rule": "compositing kernel: bound = factor * e32 + 1e-6 on the figure, factor 4 unless listed under factors; e32 = the "
                    "float32 run of tests/helpers/ngp_normals_oracle.py::normals_reference against its float64 run.  Density-"
                    "gradient chain (16-bit derivatives, no derivable bound): bound = 2.5 x the value measured on gfx950",
            "figure": "max|got - ref64| / max|ref64| over the unnormalised sums [R][3]",
            "factors": {}, "e32": {}, "measured_gfx950": {}, "chain": {}}


def main():
    m = _load_or_new()
    if "--measured" in sys.argv:
        with open(sys.argv[sys.argv.index("--measured") + 1]) as fh:
            got = json.load(fh)
        m["measured_gfx950"] = {k: v for k, v in got.items() if not k.startswith("chain/")}
        ch = {k[len("chain/"):]: v for k, v in got.items() if k.startswith("chain/")}
        if ch:
            m["chain"] = {"measured_max_angle_deg": ch["max_angle_deg"], "measured_median_angle_deg": ch["median_angle_deg"],
                          "bound_max_angle_deg": CHAIN_FACTOR * ch["max_angle_deg"],
                          "bound_median_angle_deg": CHAIN_FACTOR * ch["median_angle_deg"], "factor": CHAIN_FACTOR,
                          "floor_rel": GRAD_FLOOR_REL, "share_below_floor_ref64": ch.get("share_below_floor")}
    else:
        e32 = e32_figures()
        for k, v in e32.items():
            print(f"{k:32s} {v:.3e}")
        print(normals_case()["classes"])
        if "--write" in sys.argv:
            m["e32"] = e32
            m["factors"] = {k: {"factor": N.CAPPED_FACTOR, "reason": N.CAPPED_REASON} for k in e32 if k.endswith("_capped")}
    if "--write" in sys.argv or "--measured" in sys.argv:
        with open(MARGINS_PATH, "w") as fh:
            json.dump(m, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
