"""CPU side of the occupancy-grid back-end's normals path: the plain-torch references of tests/helpers/
ngp_normals_oracle.py agree between float32 and float64, their cases hold every class the GPU tests rely on, the
committed float32 figures (profiles/ngp_normals_parity_margins.json, what the GPU bounds are made of) are current, the
float64 density-gradient reference alone keeps the share of near-zero gradients under the test's condition, and the C ABI
carries the new entry points."""
import ctypes as C

import torch

from helpers import ngp_normals_oracle as H
from helpers import ngp_oracle as N


def test_reference_float32_agrees_with_float64():
    """float32 sums of at most ~200 terms of size <= 1: a figure far below 1e-5 (a float32 ulp is 6e-8; the exponent of a
    transmittance carries the rounding of optical depths below ~20); rays with a capped sample round at the scale of 128
    (half ulp 7.6e-6) and are judged apart"""
    e32 = H.e32_figures()
    assert e32["normals"] < 1e-5 and e32["specials/normals"] < 1e-5 and e32["specials/normals_capped"] < 1e-4, e32


def test_case_holds_every_class():
    for specials in (False, True):
        case = H.normals_case(specials=specials)
        c = case["classes"]
        for n in ("empty", "dropped", 1, 63, 64, 65, 200):
            assert c[f"count_{n}"] >= 1, n
        assert c["dropped_slots"] > 0 and c["free_slots"] > 0
        assert c["face0"] == c["face0_expected"] == 65 and c["face1"] == c["face1_expected"] == 64
        assert c["outside"] >= 20 and c["near_face"] == 0
        assert c["zero_grad"] >= 20 and c["one_axis"] >= 20
        assert c["long_surface"] >= 1 and c["long_thin"] >= 1
        assert (c["hot"] > 0 and c["fp16_max"] == 1 and c["neg_inf"] == 1 and c["dt0"] == 1) == specials
        ref = H.normals_reference(case)
        assert bool(ref["capped_ray"].any()) == specials
        live = case["ray_idx"] >= 0
        assert bool(torch.isnan(case["dx01"][~live]).all()) and bool(torch.isfinite(case["dx01"][live]).all())
        S = ref["S"]
        assert bool(torch.isfinite(S).all()) and float(S.norm(dim=1).max()) <= 1.0 + 1e-9
        for r in range(case["R"]):
            if int(case["counts"][r]) == 0:
                assert float(S[r].abs().max()) == 0.0
        # the face rays: the masked axis carries nothing
        faces = [r for r in range(case["R"]) if float(case["origins"][r].abs().max()) == 8.0]
        assert len(faces) == 2
        for r in faces:
            k = int(case["origins"][r].abs().argmax())
            assert float(S[r, k]) == 0.0 and float(S[r].abs().max()) > 0.0


def test_rounds_of_the_reference_equal_one_pass():
    case = H.normals_case()
    whole = H.normals_reference(case)["S"]
    for cut in H.ROUND_CUTS:
        (c1, o1), (c2, o2) = N.split_rounds(case, cut)
        first = H.normals_reference(case, counts=c1, offsets=o1)["S"]
        carry = H.carry_reference(case, c1, o1)
        both = H.normals_reference(case, counts=c2, offsets=o2, carry_in=carry, accumulate=first)["S"]
        assert N.figure(both, whole) < 1e-12, cut


def test_committed_float32_figures_are_current():
    """e32 recomputed against the committed file: more than 2x away (floor: one float32 ulp) fails"""
    m = H.load_margins()
    now = H.e32_figures()
    assert set(now) == set(m["e32"])
    bad = {k: (m["e32"][k], v) for k, v in now.items() if v > 2 * m["e32"][k] + 2.0 ** -23 or m["e32"][k] > 2 * v + 2.0 ** -23}
    assert not bad, bad
    assert set(m["factors"]) == {"specials/normals_capped"} and m["factors"]["specials/normals_capped"]["factor"] == N.CAPPED_FACTOR
    assert H.bound_for("normals", m) == 4 * m["e32"]["normals"] + 1e-6
    ch = m["chain"]
    assert ch["bound_max_angle_deg"] == H.CHAIN_FACTOR * ch["measured_max_angle_deg"]
    assert ch["bound_median_angle_deg"] == H.CHAIN_FACTOR * ch["measured_median_angle_deg"]


def test_gradient_reference_keeps_the_share_below_the_floor():
    """the condition of the GPU test, on the float64 reference alone: at most 5 % of the inside points below the floor;
    outside points are exact zeros, face points carry nothing on the face's axis"""
    from oracle.ngp import NgpOracle

    case = H.gradient_case(NgpOracle(aabb_scale=4).spec.n_params)
    dens, grad = H.gradient_reference(case)
    floor, share = H.gradient_floor(grad, case["kind"])
    assert floor > 0.0 and share <= H.GRAD_MAX_BELOW, (floor, share)
    k = case["kind"]
    assert float(grad[k == 2].abs().max()) == 0.0 and float(dens[k == 2].abs().max()) == 0.0
    assert bool((dens[k != 2] > 0).all())
    face = grad[k == 1]
    assert bool(((face == 0).sum(1) == 1).all())
    # the field is not flat: the density moves by more than a factor of two over the points
    assert float(dens[k == 0].max() / dens[k == 0].min()) > 2.0


def test_abi_has_the_normals_entry_points():
    from nerf_vo_amd import _lib

    lib = _lib.lib()
    assert hasattr(lib, "nvo_ngp_normal_seed") and hasattr(lib, "nvo_ngp_composite_normals")
    assert {"nvo_ngp_normal_seed", "nvo_ngp_composite_normals"} <= set(_lib.exported_symbols())
    a = _lib.NgpNormalArgs(R=0, aabb_lo=0.0, aabb_hi=1.0)
    assert lib.nvo_ngp_composite_normals(None, C.byref(a)) == 0      # (R = 0: nothing to launch)
    assert lib.nvo_ngp_normal_seed(None, 0, 16.0, None) == 0
    assert lib.nvo_ngp_composite_normals(None, None) != 0
